"""Plain references for the match search's passes after the candidate walk (enc_match.hip), and
the cases tests/test_gpu_match_passes.py runs them on.  Each pass is restated from the header
comment of its kernel, vectorised in numpy; tests/test_match_passes_host.py checks every one
against a per-position Python loop (the naive_* functions here), so that a vectorisation
mistake does not become the standard.

The records (brotli_amd.debug_match_records, include/brotli_amd.h): per position four u32,
length << 24 | distance, valid entries first.  The passes, in the encoder's order:

 walk   test_gpu_match_records.reference_records (the records every other pass starts from).

 words  (static dictionary; one-shot streams at quality >= 10 and lgwin <= 22.)  For p <
        min(65536, n) with 4 bytes left and an empty record: the first entry of p's bucket, in
        the table's fill order, whose word is no longer than `limit` (the bytes to the end of
        p's 64 KiB segment or of the stream) and matches in full: L << 24 | 1 << 23 | index.
        The table: buckets of 8 by dict_hash of a word's first four bytes, filled with lengths
        24 down to 4, indices ascending; a word that finds its bucket full is dropped.

 tail   (custom dictionary of at least 4 bytes; streams that are not stored.)  For q >= 3 where
        the four bytes ending at q are the dictionary's last four: L = the common suffix of the
        stream up to q and of the dictionary, at most 200, the dictionary's length and the bytes
        from the start of q's segment to q.  L << 24 | 0xFFFFFF is offered at q - L + 1 if that
        record is empty; of several offers to one record the longest wins.

 near   (quality >= 10 outside FONT mode; streams that are not stored.)  For p with 2 bytes left:
        reach = min(63, (1 << lgwin) - 16, p + history); d2 = the nearest d in 1..reach whose
        2 bytes equal those at p, d3 = the nearest whose 3 bytes do (the third byte must exist
        in the stream); cap = min(limit, 32).  If d2 < d3 and cap >= 2: an entry (d2, 2).  If
        d3 exists: its length is the common prefix capped at cap, an entry if that is longer
        than the entry before it (and at least 2).  Merge: a record whose first entry is a word
        or a tail copy stays as it is; otherwise the near entries, then the old entries strictly
        longer than the best near length; more than four drop from the front.

This near rule is the kernel's documented one, and it is what is pinned here.  It differs from
the reference implementation's findAllMatches, which never offers position 0 and measures to
maxLength instead of 32 bytes.

`seg` and `span` (the parse segment and the words' span, 65536 in the product) are parameters
only so that the naive cross-check reaches the seams on inputs of a few hundred bytes."""
import functools
import os

import numpy as np

import brotli_amd
from brotli_amd import datagen
from test_gpu_match_records import depth_for_quality, reference_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 1 << 16
ENTRIES = 4
NEAR = 63          # the farthest near distance
NEAR_CAP = 32      # near copies are measured up to this length
LONG_COPY = 200    # the longest custom-tail copy
WORD_FLAG = 1 << 23
TAIL_MARK = 0xFFFFFF
DICT_HASH_BITS = 15
DICT_WAYS = 8
SIZE_BITS = [0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5]
PASS_NEAR, PASS_WORDS, PASS_TAIL = 1, 2, 4
FONT = brotli_amd.EncoderMode.FONT


def lens(r):
    return r >> 24


def dists(r):
    return r & 0xFFFFFF


# ---------------------------------------------------------------- the static dictionary
@functools.lru_cache(maxsize=None)
def dictionary():
    """(words, table): words[L] the RFC 7932 words of length L as an (count, L) u8 array; table
    the (2^15, 8) bucket table of L << 16 | index in fill order, 0 = empty"""
    with open(os.path.join(ROOT, 'brotli-lib_amd', 'data', 'dictionary.bin'), 'rb') as f:
        blob = np.frombuffer(f.read(), dtype=np.uint8)
    words, off = {}, 0
    for L in range(4, 25):
        cnt = 1 << SIZE_BITS[L]
        words[L] = blob[off:off + cnt * L].reshape(cnt, L)
        off += cnt * L
    assert off == len(blob)
    table = np.zeros((1 << DICT_HASH_BITS, DICT_WAYS), dtype=np.uint32)
    fill = np.zeros(1 << DICT_HASH_BITS, dtype=np.int64)
    for L in range(24, 3, -1):
        h = dict_hash(words[L][:, :4])
        for i, b in enumerate(h.tolist()):
            if fill[b] < DICT_WAYS:
                table[b, fill[b]] = (L << 16) | i
                fill[b] += 1
    return words, table


def dict_hash(b4):
    """the bucket of four bytes (an (m, 4) u8 array): their little-endian u32 * 0x1E35A7BD >> 17"""
    b4 = np.asarray(b4, dtype=np.uint64)
    w = b4[:, 0] | (b4[:, 1] << np.uint64(8)) | (b4[:, 2] << np.uint64(16)) | (b4[:, 3] << np.uint64(24))
    return (((w * np.uint64(0x1E35A7BD)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - DICT_HASH_BITS)).astype(np.int64)


def limits(n, seg):
    """per position: the bytes to the end of its segment or of the stream"""
    p = np.arange(n, dtype=np.int64)
    return np.minimum((p // seg + 1) * seg, n) - p


def add_words(rec, data, seg=SEG, span=SEG):
    a = np.frombuffer(data, dtype=np.uint8)
    n = len(a)
    words, table = dictionary()
    m = min(span, n) if n >= 4 else 0
    p = np.flatnonzero(rec[:max(0, min(m, n - 3)), 0] == 0)
    if not p.size:
        return rec
    pad = np.concatenate([a, np.zeros(24, dtype=np.uint8)])
    win = np.lib.stride_tricks.sliding_window_view(pad, 24)
    lim = limits(n, seg)[p]
    bucket = dict_hash(win[p, :4])
    found = np.zeros(p.size, dtype=bool)
    for way in range(DICT_WAYS):
        e = table[bucket, way]
        L, idx = (e >> 16).astype(np.int64), (e & 0xFFFF).astype(np.int64)
        for wl in np.unique(L[(e != 0) & ~found]):
            s = np.flatnonzero((e != 0) & ~found & (L == wl) & (wl <= lim))
            if not s.size:
                continue
            hit = s[(win[p[s], :wl] == words[wl][idx[s]]).all(axis=1)]
            rec[p[hit], 0] = (np.uint32(wl) << np.uint32(24)) | np.uint32(WORD_FLAG) | idx[hit].astype(np.uint32)
            found[hit] = True
    return rec


def naive_words(rec, data, seg=SEG, span=SEG):
    n = len(data)
    words, table = dictionary()
    for p in range(min(span, n)):
        if p + 4 > n or rec[p, 0] != 0:
            continue
        limit = min((p // seg + 1) * seg, n) - p
        w = int.from_bytes(data[p:p + 4], 'little')
        for e in table[((w * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - DICT_HASH_BITS)].tolist():
            if e == 0:
                break
            L, idx = e >> 16, e & 0xFFFF
            if L <= limit and data[p:p + L] == words[L][idx].tobytes():
                rec[p, 0] = (L << 24) | WORD_FLAG | idx
                break
    return rec


# ---------------------------------------------------------------- the custom dictionary's tail
def add_tail(rec, data, cdict, seg=SEG):
    a = np.frombuffer(data, dtype=np.uint8)
    d = np.frombuffer(cdict, dtype=np.uint8)
    n = len(a)
    if len(d) < 4 or n < 4:
        return rec
    q = np.arange(3, n, dtype=np.int64)
    cap = np.minimum(min(LONG_COPY, len(d)), q - (q // seg) * seg + 1)
    L = np.zeros(q.size, dtype=np.int64)
    alive = np.ones(q.size, dtype=bool)
    for k in range(min(LONG_COPY, len(d))):
        alive &= (k < cap) & (q - k >= 0)
        alive[alive] = a[q[alive] - k] == d[len(d) - 1 - k]
        if not alive.any():
            break
        L[alive] = k + 1
    ok = L >= 4
    p, Lp = q[ok] - L[ok] + 1, L[ok]
    free = rec[p, 0] == 0
    best = np.zeros(n, dtype=np.int64)
    np.maximum.at(best, p[free], Lp[free])
    w = np.flatnonzero(best)
    rec[w, 0] = (best[w].astype(np.uint32) << np.uint32(24)) | np.uint32(TAIL_MARK)
    return rec


def naive_tail(rec, data, cdict, seg=SEG):
    n = len(data)
    if len(cdict) < 4:
        return rec
    walk_empty = rec[:, 0] == 0
    for q in range(3, n):
        if data[q - 3:q + 1] != cdict[-4:]:
            continue
        cap = min(LONG_COPY, len(cdict), q - (q // seg) * seg + 1)
        if cap < 4:
            continue
        L = 4
        while L < cap and data[q - L] == cdict[-1 - L]:
            L += 1
        p = q - L + 1
        if walk_empty[p] and lens(int(rec[p, 0])) < L:
            rec[p, 0] = (L << 24) | TAIL_MARK
    return rec


# ---------------------------------------------------------------- the near scan
def near_entries(buf, history, lgwin, seg=SEG):
    """(f0, f1, best) per stream position: the near entries (0: none), first one first, and the
    best near length (the merge's threshold).  buf: the history bytes, then the stream."""
    b = np.frombuffer(buf, dtype=np.uint8)
    n = len(b) - history
    f0 = np.zeros(n, dtype=np.uint32)
    f1 = np.zeros(n, dtype=np.uint32)
    best = np.ones(n, dtype=np.int64)
    if n < 2:
        return f0, f1, best
    p = np.arange(n, dtype=np.int64)
    i = p + history
    pad = np.concatenate([b.astype(np.int64), np.full(NEAR_CAP + 3, -1, dtype=np.int64)])
    reach = np.minimum(min(NEAR, (1 << lgwin) - 16), i)
    has2, has3 = p + 2 <= n, p + 3 <= n
    d2 = np.full(n, 64, dtype=np.int64)
    d3 = np.full(n, 64, dtype=np.int64)
    for d in range(NEAR, 0, -1):   # nearest last: it overwrites
        ok = (d <= reach) & has2
        j = np.where(ok, i - d, 0)
        e2 = ok & (pad[i] == pad[j]) & (pad[i + 1] == pad[j + 1])
        e3 = e2 & has3 & (pad[i + 2] == pad[j + 2])
        d2[e2] = d
        d3[e3] = d
    cap = np.minimum(limits(n, seg), NEAR_CAP)
    two = (d2 < d3) & (cap >= 2)
    f0[two] = (np.uint32(2) << np.uint32(24)) | d2[two].astype(np.uint32)
    best[two] = 2
    s = np.flatnonzero(d3 < 64)
    ln = np.zeros(s.size, dtype=np.int64)
    alive = np.ones(s.size, dtype=bool)
    for k in range(NEAR_CAP):
        alive &= (k < cap[s]) & (pad[i[s] + k] == pad[i[s] - d3[s] + k])
        ln[alive] = k + 1
    t = ln > best[s]
    s, ln = s[t], ln[t]
    w = (ln.astype(np.uint32) << np.uint32(24)) | d3[s].astype(np.uint32)
    second = f0[s] != 0
    f1[s[second]] = w[second]
    f0[s[~second]] = w[~second]
    best[s] = ln
    return f0, f1, best


def naive_near_entries(buf, history, lgwin, seg=SEG):
    n = len(buf) - history
    f0 = np.zeros(n, dtype=np.uint32)
    f1 = np.zeros(n, dtype=np.uint32)
    best = np.ones(n, dtype=np.int64)
    s = buf[history:]
    for p in range(n - 1):
        reach = min(NEAR, (1 << lgwin) - 16, p + history)
        i = p + history
        d2 = d3 = None
        for d in range(1, reach + 1):
            if buf[i - d:i - d + 2] == s[p:p + 2]:
                if d2 is None:
                    d2 = d
                if d3 is None and p + 3 <= n and buf[i - d + 2] == s[p + 2]:
                    d3 = d
                    break
        cap = min(min((p // seg + 1) * seg, n) - p, NEAR_CAP)
        out = []
        if d2 is not None and (d3 is None or d2 < d3) and cap >= 2:
            out.append((2 << 24) | d2)
            best[p] = 2
        if d3 is not None:
            ln = 0
            while ln < cap and buf[i - d3 + ln] == s[p + ln]:
                ln += 1
            if ln > best[p]:
                out.append((ln << 24) | d3)
                best[p] = ln
        if out:
            f0[p] = out[0]
        if len(out) > 1:
            f1[p] = out[1]
    return f0, f1, best


def is_copy_of_dictionary(rec, words_on):
    """records whose first entry is a custom-tail copy or (where the stream can have words) a word"""
    first = rec[:, 0]
    return (first != 0) & ((dists(first) == TAIL_MARK) | (words_on & ((first & WORD_FLAG) != 0)))


def merge_near(rec, f0, f1, best, words_on):
    """-> (records, front drops per position)"""
    out = rec.copy()
    n = len(rec)
    go = (f0 != 0) & ~is_copy_of_dictionary(rec, words_on)
    keep = (rec != 0) & (lens(rec).astype(np.int64) > best[:, None])
    cand = np.zeros((n, ENTRIES + 2), dtype=np.uint32)
    cand[:, 0], cand[:, 1] = f0, f1
    cand[:, 2:] = np.where(keep, rec, 0)
    # valid entries to the front, in order (a stable sort of "is empty")
    order = np.argsort(cand == 0, axis=1, kind='stable')
    cand = np.take_along_axis(cand, order, axis=1)
    cnt = (cand != 0).sum(axis=1)
    drop = np.where(go, np.maximum(cnt - ENTRIES, 0), 0)
    col = np.arange(ENTRIES)[None, :] + drop[:, None]
    out[go] = np.take_along_axis(cand, col, axis=1)[go]
    return out, drop


def naive_merge_near(rec, f0, f1, best, words_on):
    out = rec.copy()
    for p in range(len(rec)):
        if not f0[p]:
            continue
        first = int(rec[p, 0])
        if first and ((first & 0xFFFFFF) == TAIL_MARK or (words_on and first & WORD_FLAG)):
            continue
        w = [int(f0[p])] + ([int(f1[p])] if f1[p] else []) + [int(x) for x in rec[p] if x and (int(x) >> 24) > best[p]]
        w = w[max(0, len(w) - ENTRIES):]
        out[p] = w + [0] * (ENTRIES - len(w))
    return out


# ---------------------------------------------------------------- a call
def gates(options, history, cdict):
    """which passes an encode call with these options runs for a stream that is not stored"""
    q, lgwin = options['quality'], options.get('lgwin', 22)
    font = options.get('mode') == FONT
    words = q >= 10 and lgwin <= 22 and history == 0 and len(cdict or b'') < (1 << 22)
    return {'near': q >= 10 and not font, 'words': words, 'tail': cdict is not None and len(cdict) >= 4}


def expected_records(buf, options, passes, history=0, seg=SEG, stages=None):
    """the records of one buffer (history bytes, then the stream) after the passes asked for;
    stages (a dict): receives the walk's records and the near scan's entries"""
    data = buf[history:]
    n = len(data)
    hb = 4 if options.get('mode') == FONT else 6
    lgwin = options.get('lgwin', 22)
    rec = reference_records(data, hb, depth_for_quality(options['quality']), lgwin).copy()
    if stages is not None:
        stages['walk'] = rec.copy()
    if n < 64 or options['quality'] == 0:   # stored: no match search
        return rec
    cdict = options.get('customDictionary')
    g = gates(options, history, cdict)
    if passes & PASS_WORDS and g['words']:
        add_words(rec, data, seg)
    if passes & PASS_TAIL and g['tail']:
        add_tail(rec, data, cdict, seg)
    if stages is not None:
        stages['before_near'] = rec.copy()
    if passes & PASS_NEAR and g['near']:
        f0, f1, best = near_entries(buf, history, lgwin, seg)
        rec, drop = merge_near(rec, f0, f1, best, g['words'])
        if stages is not None:
            stages.update(f0=f0, f1=f1, best=best, drop=drop)
    return rec


# ---------------------------------------------------------------- inputs
STREAM_SIZES_SMALL = [64, 65, 66, 254, 255, 256, 257, 510, 4095, 4096, 4097]
STREAM_SIZES_SEG = [65535, 65536, 65537, 65536 + 4096 + 300]
HISTORIES = [0, 1, 3, 62, 63, 64, 200]


def few_symbols(n, seed, symbols, zeros=0):
    """n random bytes over a small alphabet; `zeros` real zero bytes at both ends"""
    rng = np.random.default_rng(seed)
    a = np.asarray(symbols, dtype=np.uint8)[rng.integers(0, len(symbols), n)]
    if zeros:
        a[:zeros] = 0
        a[n - min(zeros, n):] = 0
    return a.tobytes()


def sized_buffers(sizes, history, seed):
    """one buffer per stream size, `history` bytes in front of each; alphabets of 2 to 4 symbols
    (0 among them in most), every other buffer with zero bytes at both ends"""
    alphabets = [(0, 65), (0, 65, 66), (65, 66, 67), (0, 1, 65, 66)]
    out = []
    for k, n in enumerate(sizes):
        out.append(few_symbols(n + history, seed + k, alphabets[k % 4], zeros=(70 if k % 2 == 0 else 0)))
    return out


def periodic():
    """period-2 data and one-byte runs (the near length reaches its 32-byte cap where the walk
    has longer copies), zero runs among them, and short pieces between that break the period"""
    rng = np.random.default_rng(11)
    parts = [b'\0' * 300]
    for k in range(40):
        parts.append([b'ab', b'\0\0', b'xx', b'\0z'][k % 4] * int(rng.integers(10, 400)))
        parts.append(few_symbols(int(rng.integers(1, 9)), 100 + k, (0, 97, 98, 120)))
    parts.append(b'\0' * 300)
    return b''.join(parts)


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def word(L, idx):
    return dictionary()[0][L][idx].tobytes()


@functools.lru_cache(maxsize=None)
def dropped_word():
    """(L, idx) of a word the table dropped (its bucket was full) that no word of its bucket
    is a prefix of: looked up at a position, nothing may be found"""
    words, table = dictionary()
    for L in range(12, 3, -1):
        for idx in range(len(words[L])):
            w = words[L][idx]
            bucket = table[dict_hash(w[None, :4])[0]]
            if ((L << 16) | idx) in bucket.tolist():
                continue
            if all(e == 0 or not (e >> 16 <= L and words[e >> 16][e & 0xFFFF].tobytes() == w[:e >> 16].tobytes())
                   for e in bucket.tolist()):
                return L, idx
    raise AssertionError('no dropped word')


@functools.lru_cache(maxsize=None)
def tabled_word(L, skip=0):
    """the index of a word of length L that is in the table and is its bucket's first entry"""
    words, table = dictionary()
    for idx in range(len(words[L])):
        if table[dict_hash(words[L][idx][None, :4])[0], 0] == ((L << 16) | idx):
            if skip == 0:
                return idx
            skip -= 1
    raise AssertionError('no word of length %d' % L)


@functools.lru_cache(maxsize=None)
def word_streams():
    """(buffers, marks): random bytes (no window matches to speak of) with dictionary words placed
    in them, every placement a word of its own unless said otherwise; marks name the (stream,
    position) of a placement"""
    def W(L, k):   # the k-th word of length L that leads its bucket
        return word(L, tabled_word(L, k))

    def build(n, seed, places):
        a = bytearray(random_bytes(n, seed))
        for p, w in places:
            a[p:p + len(w)] = w
        return bytes(a)

    marks = {}
    dl, di = dropped_word()
    # stream 0: one segment
    n0 = 30000
    ctx = W(12, 1) + b'#context#'   # a word with the same bytes after it, twice: the second time the window has it
    s0 = build(n0, 21, [
        (100, W(9, 0)), (500, W(12, 0)), (900, W(6, 0)), (1300, W(4, 0)), (1700, W(24, 0)),
        (2000, ctx), (2300, ctx),
        (3000, word(dl, di)),
        (4000, W(9, 1)[:2] + b'\xfe' + W(9, 1)),   # the word's first pair 3 back: a near 2-byte copy at the word
        (n0 - 15, W(15, 0)),                          # ends exactly at the stream's end
    ])
    marks.update(plain=(0, 100), first=(0, 2000), second=(0, 2300), dropped=(0, 3000), near_pair=(0, 4003), at_end=(0, n0 - 15))
    # stream 1: the word at its end is cut by a byte
    n1 = 5000
    s1 = build(n1 + 1, 22, [(700, W(9, 2)), (n1 - 14, W(15, 1))])[:n1]
    marks.update(cut=(1, n1 - 14))
    # stream 2: across the segment's end by one byte (the whole word is there), and past the span
    n2 = SEG + 3000
    s2 = build(n2, 23, [(300, W(12, 2)), (SEG - 11, W(12, 3)), (SEG + 1000, W(15, 2))])
    marks.update(cross_seg=(2, SEG - 11), past_span=(2, SEG + 1000))
    return [s0, s1, s2], marks


TAIL_DICT = datagen.enwik_text(300, 9)
PERIODIC_DICT = b'ab' * 20


@functools.lru_cache(maxsize=None)
def tail_streams():
    """(buffers, marks) for TAIL_DICT; marks: (stream, position, the tail copy's length there, 0
    for none).  Its suffix in the first bytes of a stream; the whole dictionary (cut at 200);
    across a segment start (cut there); four bytes; at the stream's end; twice (the window has
    the second); in a stored stream."""
    d = TAIL_DICT
    marks = {}
    a = bytearray(random_bytes(3000, 31))
    a[0:50] = d[-50:]
    a[1000:1300] = d
    marks.update(start=(0, 0, 50), full=(0, 1100, 200))
    b = bytearray(random_bytes(SEG + 4000, 32))
    b[SEG - 15:SEG + 25] = d[-40:]
    b[SEG + 100:SEG + 104] = d[-4:]
    marks.update(seam=(1, SEG, 25), before_seam=(1, SEG - 15, 0), four=(1, SEG + 100, 4))
    c = bytearray(random_bytes(3000, 33))
    c[10:40] = d[-30:]
    c[7:9] = d[-30:-28]   # the copy's first pair 3 back: a near 2-byte copy where the tail copy is
    c[500:530] = d[-30:]
    marks.update(once=(2, 10, 30), twice=(2, 500, 0))
    e = random_bytes(281, 35) + d[-19:]
    marks.update(end=(3, 281, 19))
    f = d[-3:] + random_bytes(40, 34) + d[-8:]   # stored: no records
    return [bytes(a), bytes(b), bytes(c), e, f], marks


@functools.lru_cache(maxsize=None)
def periodic_tail_streams():
    """for PERIODIC_DICT: several q offer one position, the longest wins"""
    a = bytearray(random_bytes(2000, 41))
    a[0:20] = b'ab' * 10
    a[500:560] = b'ab' * 30
    return [bytes(a)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(buffers, options, passes, history)"""
    if name.startswith('small_h'):
        h = int(name[7:])
        return sized_buffers(STREAM_SIZES_SMALL, h, 1000 + h), {'quality': 11}, PASS_NEAR, h
    if name.startswith('seg_a_h'):
        h = int(name[7:])
        return sized_buffers(STREAM_SIZES_SEG[:2], h, 2000 + h), {'quality': 11}, PASS_NEAR, h
    if name.startswith('seg_b_h'):
        h = int(name[7:])
        return sized_buffers(STREAM_SIZES_SEG[2:], h, 3000 + h), {'quality': 10}, PASS_NEAR, h
    if name == 'periodic':
        return [periodic(), periodic()[5:3000]], {'quality': 11}, PASS_NEAR, 0
    if name == 'full_records':
        return [few_symbols(50000, 5, (0, 65, 66, 67), zeros=100), few_symbols(9000, 6, (65, 66))], {'quality': 11}, PASS_NEAR, 0
    if name.startswith('mixed_'):
        q, lgwin = {'mixed_q10_lgwin10': (10, 10), 'mixed_q11_lgwin22': (11, 22), 'mixed_q10_lgwin22': (10, 22),
                    'mixed_q11_lgwin10': (11, 10)}[name]
        return [datagen.enwik_text(40000, 3), random_bytes(30000, 8)], {'quality': q, 'lgwin': lgwin}, PASS_NEAR | PASS_WORDS, 0
    if name in ('words_q10', 'words_q11', 'words_near_q11', 'words_lgwin24', 'words_q9'):
        opt = {'words_q10': {'quality': 10}, 'words_lgwin24': {'quality': 11, 'lgwin': 24}, 'words_q9': {'quality': 9}}.get(name, {'quality': 11})
        return word_streams()[0], opt, PASS_WORDS | (PASS_NEAR if name == 'words_near_q11' else 0), 0
    if name == 'words_history':
        return [b'\0' * 7 + b for b in word_streams()[0][:2]], {'quality': 11}, PASS_WORDS, 7
    if name in ('tail', 'tail_near', 'tail_q5'):
        opt = {'quality': 5 if name == 'tail_q5' else 11, 'customDictionary': TAIL_DICT}
        return tail_streams()[0], opt, PASS_TAIL | (PASS_NEAR if name == 'tail_near' else 0), 0
    if name == 'tail_all_history':
        return [TAIL_DICT[-64:] + b for b in tail_streams()[0]], {'quality': 11, 'customDictionary': TAIL_DICT}, 7, 64
    if name == 'tail_periodic':
        return periodic_tail_streams(), {'quality': 11, 'customDictionary': PERIODIC_DICT}, PASS_TAIL | PASS_NEAR, 0
    if name == 'tail_short_dict':
        return tail_streams()[0], {'quality': 11, 'customDictionary': TAIL_DICT[-3:]}, PASS_TAIL, 0
    if name == 'tail_five_byte_dict':
        return tail_streams()[0], {'quality': 11, 'customDictionary': TAIL_DICT[-5:]}, PASS_TAIL, 0
    if name in ('gate_q9', 'gate_font'):
        opt = {'quality': 9} if name == 'gate_q9' else {'quality': 11, 'mode': FONT}
        return sized_buffers([300, 4097, 20000], 0, 77), opt, PASS_NEAR, 0
    raise KeyError(name)


CASES = (['small_h%d' % h for h in HISTORIES] + ['seg_a_h0', 'seg_a_h3', 'seg_b_h0', 'seg_b_h200', 'periodic', 'full_records',
         'mixed_q10_lgwin10', 'mixed_q11_lgwin22', 'mixed_q10_lgwin22', 'mixed_q11_lgwin10',
         'words_q10', 'words_q11', 'words_near_q11', 'words_lgwin24', 'words_q9', 'words_history',
         'tail', 'tail_near', 'tail_q5', 'tail_all_history', 'tail_periodic', 'tail_short_dict', 'tail_five_byte_dict',
         'gate_q9', 'gate_font'])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records per stream, stages per stream)"""
    bufs, opt, passes, history = case(name)
    recs, stages = [], []
    for b in bufs:
        st = {}
        recs.append(expected_records(b, opt, passes, history, stages=st))
        stages.append(st)
    return recs, stages
