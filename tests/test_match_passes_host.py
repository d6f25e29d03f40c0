"""The references of tests/_match_passes.py, without a GPU: each vectorised pass against a naive
per-position loop on inputs of a few hundred bytes (with a 128-byte segment, so the seams are in
them), and the conditions the GPU cases are there for, counted on the references' records alone."""
import functools

import numpy as np
import pytest

import _match_passes as mp
from _match_passes import ENTRIES, SEG, TAIL_MARK, WORD_FLAG, dists, lens

SMALL_SEG = 128


def small_inputs():
    out = []
    for seed, syms in enumerate([(0, 65), (0, 65, 66), (65, 66, 67), (0, 1, 65, 66)]):
        out.append(mp.few_symbols(300 + 37 * seed, 50 + seed, syms, zeros=(20 if seed % 2 else 0)))
    out.append(mp.periodic()[280:700])
    out.append(mp.datagen.enwik_text(500, 4))
    out.append(b'ab' * 100 + b'abc' * 60)
    return out


def walk_like(data, seed):
    """records as a walk could leave them: increasing lengths of 4 and more, some full, some empty"""
    rng = np.random.default_rng(seed)
    n = len(data)
    rec = np.zeros((n, ENTRIES), dtype=np.uint32)
    cnt = rng.integers(0, ENTRIES + 1, n)
    ln = np.sort(rng.integers(4, 40, (n, ENTRIES)), axis=1)
    ln += np.arange(ENTRIES)[None, :]   # strictly increasing
    d = rng.integers(64, 4000, (n, ENTRIES))
    w = (ln.astype(np.uint32) << np.uint32(24)) | d.astype(np.uint32)
    for c in range(1, ENTRIES + 1):
        rec[cnt == c, :c] = w[cnt == c, ENTRIES - c:]
    return rec


@pytest.mark.parametrize('history', [0, 1, 3, 62, 63, 64, 200])
def test_near_entries_against_the_loop(history):
    one = two = 0
    for k, data in enumerate(small_inputs()):
        buf = mp.few_symbols(history, 900 + k, (0, 65, 66)) + data
        for lgwin in (10, 22):
            got = mp.near_entries(buf, history, lgwin, SMALL_SEG)
            want = mp.naive_near_entries(buf, history, lgwin, SMALL_SEG)
            for g, w, what in zip(got, want, ('f0', 'f1', 'best')):
                assert (g == w).all(), (history, k, what, np.flatnonzero(g != w)[:5])
        one += int((got[0] != 0).sum())
        two += int((got[1] != 0).sum())
    assert one > 500 and two > 50


def test_near_merge_against_the_loop():
    drops = np.zeros(3, dtype=np.int64)
    for k, data in enumerate(small_inputs()):
        f0, f1, best = mp.near_entries(data, 0, 22, SMALL_SEG)
        rec = walk_like(data, k)
        rec[5::17, 0] = (9 << 24) | WORD_FLAG | 77   # words and tail copies: the only entry
        rec[5::17, 1:] = 0
        rec[11::23, 0] = (30 << 24) | TAIL_MARK
        rec[11::23, 1:] = 0
        for words_on in (True, False):
            got, drop = mp.merge_near(rec, f0, f1, best, words_on)
            want = mp.naive_merge_near(rec, f0, f1, best, words_on)
            assert (got == want).all(), (k, words_on, np.flatnonzero((got != want).any(axis=1))[:5])
        drops += np.bincount(drop, minlength=3)
    assert (drops > 20).all()


def test_words_against_the_loop():
    texts = [mp.datagen.enwik_text(700, s) for s in (1, 2, 3)]
    texts.append(mp.word(9, mp.tabled_word(9)) * 3 + b'the time of their lives' + mp.word(*mp.dropped_word()) + b' information')
    for k, data in enumerate(texts):
        rec = np.zeros((len(data), ENTRIES), dtype=np.uint32)
        rec[3::7, 0] = (5 << 24) | 100   # the window has a match here
        got = mp.add_words(rec.copy(), data, SMALL_SEG, 256)
        want = mp.naive_words(rec.copy(), data, SMALL_SEG, 256)
        assert (got == want).all(), (k, np.flatnonzero((got != want).any(axis=1))[:5])
        assert ((got[:, 0] & WORD_FLAG) != 0).sum() >= 3
        assert (got[256:, 0] == rec[256:, 0]).all()


def test_tail_against_the_loop():
    d = mp.TAIL_DICT
    rng = np.random.default_rng(3)
    for k, cdict in enumerate([d, d[-5:], d[-4:], d[-3:], mp.PERIODIC_DICT, b'\0' * 250]):
        a = bytearray(mp.random_bytes(900, 60 + k))
        for _ in range(12):
            L = int(rng.integers(1, min(len(cdict), 260) + 1))
            p = int(rng.integers(0, 900 - L))
            a[p:p + L] = cdict[-L:]
        a[120:135] = (cdict * 8)[-15:]   # across a segment start
        data = bytes(a)
        rec = np.zeros((len(data), ENTRIES), dtype=np.uint32)
        rec[3::7, 0] = (5 << 24) | 100
        got = mp.add_tail(rec.copy(), data, cdict, SMALL_SEG)
        want = mp.naive_tail(rec.copy(), data, cdict, SMALL_SEG)
        assert (got == want).all(), (k, np.flatnonzero((got != want).any(axis=1))[:5])
        assert (dists(got[:, 0]) == TAIL_MARK).any() == (len(cdict) >= 4)


# ---------------------------------------------------------------- what the GPU cases reach
def test_size_cases_reach_the_seams():
    for name in [c for c in mp.CASES if c.startswith(('small_h', 'seg_a_h', 'seg_b_h'))]:
        bufs, opt, passes, history = mp.case(name)
        recs, stages = mp.expected(name)
        two_only = three_only = both = drops = tile = block_last = block_first = seg_last = seg_first = 0
        for b, st in zip(bufs, stages):
            n = len(b) - history
            f0, f1, drop = st['f0'], st['f1'], st['drop']
            p = np.arange(n)
            has = f0 != 0
            two_only += int((has & (f1 == 0) & (lens(f0) == 2)).sum())
            three_only += int((has & (f1 == 0) & (lens(f0) >= 3)).sum())
            both += int((f1 != 0).sum())
            drops += int((drop > 0).sum())
            in_block = p % 4096
            tile += int((has & (in_block % 255 == 254)).sum()) and int((has & (in_block % 255 == 0) & (in_block > 0)).sum())
            block_last += int((has & (in_block == 4095)).sum())
            block_first += int((has & (in_block == 0) & (p > 0)).sum())
            seg_last += int((has[SEG - 2:SEG]).sum()) if n > SEG else 0
            seg_first += int((has[SEG:SEG + 1]).sum()) if n > SEG else 0
        sizes = [len(b) - history for b in bufs]
        assert two_only and three_only and both, name
        if max(sizes) > 254:
            assert tile, name
        if max(sizes) > 4096:   # (4097: the pair after the block's last position is cut by the stream's end)
            assert block_last and drops, name
        if max(sizes) > 4098:
            assert block_first, name
        if name.startswith('seg_b') or max(sizes) > SEG:
            assert seg_last and seg_first, name
    # every stream size and history of the list is in some case
    seen = set()
    for name in mp.CASES:
        bufs, _, _, history = mp.case(name)
        seen.update((len(b) - history, history) for b in bufs)
    for n in mp.STREAM_SIZES_SMALL:
        for h in mp.HISTORIES:
            assert (n, h) in seen
    for n in mp.STREAM_SIZES_SEG:
        assert any((n, h) in seen for h in mp.HISTORIES)


def test_segment_seam_positions():
    """one and two bytes before a segment's end the cap is 1 and 2: no entry, and 2-byte entries
    only, while the pair at the next position lies in the next segment"""
    for name in ('seg_b_h0', 'seg_b_h200', 'seg_a_h0'):
        for b, st in zip(mp.case(name)[0], mp.expected(name)[1]):
            n = len(b) - mp.case(name)[3]
            if n <= SEG:
                # (the stream's end instead: nothing in the last position, at most 2 bytes before it)
                assert st['f0'][n - 1] == 0 and lens(st['f0'][n - 2]) in (0, 2)
                continue
            assert st['f0'][SEG - 1] == 0 and st['f1'][SEG - 1] == 0
            assert lens(st['f0'][SEG - 2]) == 2 and st['f1'][SEG - 2] == 0
    assert any(lens(st['f0'][SEG - 3]) == 3 for name in ('seg_b_h0', 'seg_b_h200') for st in mp.expected(name)[1])


def test_zero_padding_is_not_data():
    """streams that start and end in real zero bytes: the first position has no entry (nothing
    lies before it), the second one has (the zero before it is data)"""
    bufs, _, _, history = mp.case('small_h0')
    st = mp.expected('small_h0')[1]
    for k in (2, 8, 10):   # 66, 4095 and 4097 bytes
        b, n = bufs[k], len(bufs[k])
        assert b[:33] == b'\0' * 33 and b[-33:] == b'\0' * 33
        assert st[k]['f0'][0] == 0 and st[k]['f0'][1] == ((32 << 24) | 1)
        assert st[k]['f0'][n - 2] == ((2 << 24) | 1) and st[k]['f0'][n - 1] == 0 and st[k]['f0'][n - 3] == ((3 << 24) | 1)
    # with a history, position 0 reaches back into it
    st = mp.expected('small_h3')[1]
    assert st[8]['f0'][0] == ((32 << 24) | 1)


def test_periodic_and_full_records():
    recs, stages = mp.expected('periodic')
    st = stages[0]
    # the near length at its cap where the walk has a longer copy, kept behind it
    capped = (lens(st['f0']) == 32) | (lens(st['f1']) == 32)
    longer = lens(st['walk']).max(axis=1) > 32
    assert (capped & longer).sum() > 100
    both = np.flatnonzero(capped & longer)
    assert all(lens(recs[0][p]).max() > 32 and lens(recs[0][p][0]) <= 32 for p in both[:50])
    recs, stages = mp.expected('full_records')
    st = stages[0]
    full = (st['walk'] != 0).all(axis=1)
    # four tree entries, all longer than a 2-byte and a 3+-byte near entry: two dropped from the front
    assert ((st['drop'] == 2) & full & (st['f1'] != 0) & (lens(st['walk'][:, 0]) > st['best'])).sum() > 10
    assert (st['drop'] == 1).sum() > 10
    # tree entries no longer than the near copy are replaced by it
    assert ((lens(st['walk'][:, 0]) <= st['best']) & (st['walk'][:, 0] != 0) & (st['f0'] != 0)).sum() > 10


def test_mixed_cases():
    for name in ('mixed_q10_lgwin10', 'mixed_q11_lgwin22', 'mixed_q10_lgwin22', 'mixed_q11_lgwin10'):
        recs, stages = mp.expected(name)
        for r, st in zip(recs, stages):
            assert (st['f0'] != 0).sum() >= 20, name
            assert (r != st['walk']).any(axis=1).sum() >= 20, name
        assert ((recs[0][:, 0] & WORD_FLAG) != 0).sum() > 100, name   # text: words
    a, b = mp.expected('mixed_q11_lgwin10')[0], mp.expected('mixed_q11_lgwin22')[0]
    assert (a[0] != b[0]).any()
    a, b = mp.expected('mixed_q10_lgwin22')[0], mp.expected('mixed_q11_lgwin22')[0]
    assert (a[0] != b[0]).any()


def is_word(w, L=None):
    return w != 0 and dists(w) != TAIL_MARK and (w & WORD_FLAG) != 0 and (L is None or lens(w) == L)


def test_word_cases():
    bufs, marks = mp.word_streams()
    for name in ('words_q10', 'words_q11', 'words_near_q11'):
        recs, stages = mp.expected(name)

        def first(mark):
            s, p = marks[mark]
            return int(recs[s][p, 0]), [int(x) for x in recs[s][p, 1:]], stages[s]

        for mark, L in (('plain', 9), ('first', 12), ('at_end', 15), ('near_pair', 9)):
            w, rest, _ = first(mark)
            assert is_word(w, L) and rest == [0, 0, 0], (name, mark)
        w, _, st = first('second')
        s, p = marks['second']
        assert not is_word(w) and st['walk'][p, 0] != 0   # the window already has a match there
        for mark, L in (('cut', 15), ('cross_seg', 12), ('past_span', 15)):
            assert not is_word(first(mark)[0], L), (name, mark)
        assert not is_word(first('past_span')[0])
        s, p = marks['cross_seg']   # the whole word is in the stream, its last byte in the next segment
        assert p + 12 == SEG + 1 and mp.add_words(np.zeros((13, ENTRIES), np.uint32), bufs[s][p:p + 13])[0, 0] >> 24 == 12
        s, p = marks['dropped']
        dl, di = mp.dropped_word()
        assert bufs[s][p:p + dl] == mp.word(dl, di) and not is_word(int(recs[s][p, 0])) and stages[s]['before_near'][p, 0] == 0
        if name == 'words_near_q11':
            s, p = marks['near_pair']
            assert stages[s]['f0'][p] == ((2 << 24) | 3)   # the near 2-byte copy the word's record does not take
    # the ninth word of a bucket: in the dictionary, not in the table
    words, table = mp.dictionary()
    dl, di = mp.dropped_word()
    bucket = table[mp.dict_hash(words[dl][di][None, :4])[0]]
    assert (bucket != 0).all() and ((dl << 16) | di) not in bucket.tolist()
    # the gates: no word at lgwin 24, at q9, or behind a history
    for name in ('words_lgwin24', 'words_q9', 'words_history'):
        recs, stages = mp.expected(name)
        assert all((r == st['walk']).all() for r, st in zip(recs, stages)), name
        bufs_g, opt, passes, history = mp.case(name)
        open_ = mp.add_words(stages[0]['walk'].copy(), bufs_g[0][history:])
        assert (open_ != stages[0]['walk']).any(), name   # (without the gate there would be words)


def test_tail_cases():
    bufs, marks = mp.tail_streams()
    for name in ('tail', 'tail_near', 'tail_q5', 'tail_all_history'):
        recs, stages = mp.expected(name)
        for mark, (s, p, L) in marks.items():
            w = int(recs[s][p, 0])
            if L:
                assert w == ((L << 24) | TAIL_MARK) and (recs[s][p, 1:] == 0).all(), (name, mark)
            else:
                assert dists(w) != TAIL_MARK, (name, mark)
        assert (recs[4] == 0).all()   # stored
        s, p, _ = marks['twice']
        assert stages[s]['walk'][p, 0] != 0
        if name in ('tail_near', 'tail_all_history'):
            # a tail copy where the near scan has an entry stays alone
            assert any(((dists(r[:, 0]) == TAIL_MARK) & (st['f0'] != 0)).any() for r, st in zip(recs[:4], stages[:4])), name
    recs, stages = mp.expected('tail_short_dict')
    assert all((r == st['walk']).all() for r, st in zip(recs, stages))
    recs, _ = mp.expected('tail_five_byte_dict')
    tails = np.concatenate([r[:, 0][dists(r[:, 0]) == TAIL_MARK] for r in recs])
    assert set(lens(tails).tolist()) == {4, 5}
    recs, _ = mp.expected('tail_periodic')
    assert recs[0][0, 0] == ((20 << 24) | TAIL_MARK)   # offered with 4, 6, .. 20 bytes: the longest


def test_gate_cases():
    for name in ('gate_q9', 'gate_font'):
        bufs, opt, passes, history = mp.case(name)
        recs, stages = mp.expected(name)
        assert passes == mp.PASS_NEAR and all((r == st['walk']).all() and 'f0' not in st for r, st in zip(recs, stages))
        f0, _, _ = mp.near_entries(bufs[2], 0, 22)
        assert (f0 != 0).sum() > 1000   # (without the gate the scan would have entries)


def test_entry_refuses_unknown_passes_and_short_buffers():
    with pytest.raises(mp.brotli_amd.BrotliError):
        mp.brotli_amd.debug_match_records([b'x' * 100], {'quality': 11}, passes=8)
    with pytest.raises(mp.brotli_amd.BrotliError):
        mp.brotli_amd.debug_match_records([b'x' * 100, b'x' * 5], {'quality': 11}, passes=1, history=6)


# the GPU test of a case asserts these as well (once a process): what the case is there for
REACHES = {
    'small_h': (test_size_cases_reach_the_seams, test_zero_padding_is_not_data),
    'seg_': (test_size_cases_reach_the_seams, test_segment_seam_positions),
    'periodic': (test_periodic_and_full_records,),
    'full_records': (test_periodic_and_full_records,),
    'mixed_': (test_mixed_cases,),
    'words_': (test_word_cases,),
    'tail': (test_tail_cases,),
    'gate_': (test_gate_cases,),
}


@functools.lru_cache(maxsize=None)
def _once(check):
    check()
    return True


def reached(name):
    checks = [c for prefix, cs in REACHES.items() if name.startswith(prefix) for c in cs]
    assert checks, name
    return all(_once(c) for c in checks)
