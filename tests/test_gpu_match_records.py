"""The match finder's records (find_matches_kernel, enc_match.hip) against a plain numpy
restatement of the rules in the kernel's header comment, exactly:

 1. the candidates of position g are the earlier positions of the same stream with the same
    17-bit hashn key (collisions included), nearest first; at most min(depth, 64) are examined,
    ending at the first one farther than (1 << lgwin) - 16;
 2. len is the common prefix, capped at min(bytes to the end of g's 64 KiB segment or of the
    stream, 255);
 3. a candidate is taken if len > best; best starts at 3;
 4. the last four taken are kept, longest last;
 5. the walk ends after a take with len >= that cap;
 6. positions with fewer than hash_bytes bytes left have empty records.

mib_debug_match_records runs an encode call's bucket sort and find_matches only, so the records
are the walk's own (no near scan, no dictionary entries)."""
import functools

import numpy as np
import pytest

import brotli_amd
from brotli_amd import datagen

HASH_BITS = 17
SEG = 1 << 16
SAT = 255
BACK = 64
ENTRIES = 4


def depth_for_quality(q):
    return 64 if q >= 11 else 32 if q == 10 else 16 if q >= 5 else 4 if q >= 2 else 1


def words_at(data, pad):
    """w[i] = the 8 bytes at i as a little-endian u64 (zeros past the end), i < len + pad"""
    n = len(data)
    b = np.zeros(n + pad + 8, dtype=np.uint64)
    b[:n] = np.frombuffer(data, dtype=np.uint8)
    w = np.zeros(n + pad, dtype=np.uint64)
    for j in range(8):
        w |= b[j:j + n + pad] << np.uint64(8 * j)
    return w


def reference_records(data, hash_bytes, depth, lgwin):
    n = len(data)
    out = np.zeros((n, ENTRIES), dtype=np.uint32)
    if n < 64:   # (stored uncompressed: no match search)
        return out
    max_dist = (1 << lgwin) - 16
    w = words_at(data, SAT + 16)
    nk = n - hash_bytes + 1   # rule 6: positions with a key
    v = w[:nk] << np.uint64(64 - 8 * hash_bytes)
    key = ((v * np.uint64(0x1E35A7BD1E35A7BD)) >> np.uint64(64 - HASH_BITS)).astype(np.int64)
    order = np.argsort(key, kind='stable')   # runs of equal keys, positions ascending
    skey = key[order]
    first = np.ones(nk, dtype=bool)
    first[1:] = skey[1:] != skey[:-1]
    run_start = np.maximum.accumulate(np.where(first, np.arange(nk), 0))
    g = order   # the position of sorted entry i
    cap = np.minimum(np.minimum((g // SEG + 1) * SEG, n) - g, SAT)   # rule 2
    best = np.full(nk, 3, dtype=np.int64)
    live = np.ones(nk, dtype=bool)
    stair = np.zeros((nk, ENTRIES), dtype=np.uint32)   # right-aligned while walking
    idx = np.arange(nk)
    for t in range(1, min(depth, BACK) + 1):   # rule 1
        live &= idx - t >= run_start
        if not live.any():
            break
        a = idx[live]
        c = g[a - t]
        dist = g[a] - c
        far = dist > max_dist
        live[a[far]] = False
        a, c, dist = a[~far], c[~far], dist[~far]
        # common prefix by 8-byte words, only as far as the cap
        ln = cap[a].copy()
        open_ = np.arange(len(a))
        off = 0
        while len(open_) and off < SAT:
            x = w[g[a[open_]] + off] ^ w[c[open_] + off]
            diff = x != 0
            fb = (x[diff].view(np.uint8).reshape(-1, 8) != 0).argmax(axis=1)
            ln[open_[diff]] = np.minimum(off + fb, cap[a[open_[diff]]])
            open_ = open_[~diff]
            open_ = open_[cap[a[open_]] > off + 8]
            off += 8
        tk = ln > best[a]   # rule 3
        at, lt, dt = a[tk], ln[tk], dist[tk]
        best[at] = lt
        stair[at, :-1] = stair[at, 1:]   # rule 4
        stair[at, -1] = (lt.astype(np.uint32) << np.uint32(24)) | dt.astype(np.uint32)
        live[at[lt >= cap[at]]] = False   # rule 5
    for _ in range(ENTRIES - 1):   # valid entries first, zeros after
        sh = (stair[:, 0] == 0) & stair.any(axis=1)
        stair[sh] = np.roll(stair[sh], -1, axis=1)
    out[g] = stair
    return out


def growing_runs():
    """one 6-gram 400 times, each followed by a shared continuation cut at a sawtooth of
    lengths (walking back from the top of a tooth every candidate is one byte longer: more
    than four takes) and a tag no other occurrence has"""
    common = bytes(range(97, 97 + 26)) + bytes(range(65, 65 + 26))
    parts = []
    for i in range(400):
        parts.append(b'#{<[(|' + common[:39 - i % 40] + b'%03d' % i)
    return b''.join(parts)


@functools.lru_cache(maxsize=None)
def case(name):
    """(buffers, options)"""
    text = datagen.enwik_text(70001, 5)
    if name == 'text':
        return [datagen.enwik_text(32768, 3)], {'quality': 11}
    if name == 'runs':
        return [growing_runs()], {'quality': 11}
    if name == 'period':
        rng = np.random.default_rng(7)
        unit = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
        n = 65536 + 2048
        return [(unit * (n // 1000 + 1))[:n]], {'quality': 11}
    if name == 'runs_lgwin10':
        return [growing_runs()], {'quality': 11, 'lgwin': 10}
    if name == 'batch':
        # (the same text in each: equal keys on both sides of every stream boundary)
        return [text, text[:300], text[:24576]], {'quality': 11}
    if name == 'text_font':
        return [datagen.enwik_text(32768, 3)], {'quality': 11, 'mode': brotli_amd.EncoderMode.FONT}
    if name == 'text_q5':
        return [datagen.enwik_text(32768, 3)], {'quality': 5}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    bufs, opt = case(name)
    hb = 4 if opt.get('mode') == brotli_amd.EncoderMode.FONT else 6
    return [reference_records(b, hb, depth_for_quality(opt['quality']), opt.get('lgwin', 22)) for b in bufs]


CASES = ['text', 'runs', 'period', 'runs_lgwin10', 'batch', 'text_font', 'text_q5']


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_match_records(name):
    bufs, opt = case(name)
    got = brotli_amd.debug_match_records(bufs, opt)
    want = expected(name)
    assert len(got) == len(want)
    for s, (gt, wt) in enumerate(zip(got, want)):
        assert gt.shape == wt.shape, (name, s)
        bad = np.flatnonzero((gt != wt).any(axis=1))
        assert bad.size == 0, '%s stream %d: %d of %d records differ, first at %d: got %s want %s' % (
            name, s, bad.size, len(wt), bad[0], [hex(x) for x in gt[bad[0]]], [hex(x) for x in wt[bad[0]]])


def test_cases_exercise_the_walk():
    """the inputs reach what they are there for (checked on the reference alone)"""
    def lens(r):
        return r >> 24

    runs = expected('runs')[0]
    assert (runs != 0).sum(axis=1).max() == ENTRIES   # a full staircase: more than four takes somewhere
    assert ((runs[:, -1] != 0) & (lens(runs[:, 0]) + 3 <= lens(runs[:, -1]))).any()
    period = expected('period')[0]
    assert (lens(period).max(axis=1) == SAT).any()   # saturation
    cut = lens(period[SEG - 200:SEG - 3]).max(axis=1)
    assert (cut == np.arange(200, 3, -1)).all()   # copies cut at the segment end
    assert (period[SEG - 3:SEG] == 0).all()   # (three bytes to the end: nothing longer than best)
    assert ((lens(period) > 32) & (lens(period) < SAT)).any()   # past the staged bytes
    near = expected('runs_lgwin10')[0]
    assert (near != runs).any() and ((near & 0xFFFFFF).max() <= (1 << 10) - 16)
    b = expected('batch')
    assert (b[1][:200] != 0).any() and ((b[1] & 0xFFFFFF) < 300).all()   # never into the stream before
    assert (expected('text_font')[0] != expected('text')[0]).any()
    assert (expected('text_q5')[0] != expected('text')[0]).any()
