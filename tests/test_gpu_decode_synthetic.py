"""The HIP decoder on written streams (tests/_streams.py), byte-exact against the model (the
oracle for static-dictionary words), through every placement of a metablock's prefix-code tables.

Which build of the decode kernel a launch gets is not observable through the ABI; these tests
rest on the rule the code states.  runtime.cpp waves_per_cu() gives ceil(streams / CUs), clamped
to 1..4, and decode.hip mib_decode_launch() launches the one-stream-per-CU ("BIG") build when
that is 1, else the four-per-CU ("batch") build.  So brotliDecode, and a decode_batch of no more
streams than the device has CUs, run BIG (table area kLdsTabBig entries, block-type trees in
LDS); a batch of more streams than CUs runs the batch build (kLdsTab = 12,224 entries,
block-type trees in scratch).  In either, a metablock whose three tree groups total no more
than the table area decodes from 16-bit LDS tables (fast_loop / hot_loop<true>), a larger one
from the HBM tables (hot_loop<false>, ctx_tree_base).  The totals of the streams used here are
asserted from the oracle decoder's own count in test_stream_builder.py.
"""
import random

import pytest

import _oracle
import _streams as S
import brotli_amd

pytestmark = pytest.mark.gpu

_cache = {}


def _cases():
    """[(name, stream bytes, expected bytes)]: the model's bytes, the oracle's for word references"""
    if 'cases' not in _cache:
        out = []
        for st, b in S.corpus():
            exp = S.model(st)
            if exp is None:
                exp = _oracle.decode(b.data)
                assert isinstance(exp, bytes)
            out.append((st.name, b.data, exp))
        _cache['cases'] = out
    return _cache['cases']


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _large_batch(extra=()):
    """more streams than CUs (the batch build): 2 * CUs + 3, the set repeated and shuffled"""
    n = 2 * _cus() + 3
    assert n <= 2048, 'beyond the decode grid cap every block decodes several streams'
    cases = list(extra) + _cases()
    picked = [cases[i % len(cases)] for i in range(max(n, len(extra) + 60))]
    assert len(picked) <= 2048
    random.Random(11).shuffle(picked)
    return picked


def _got(r):
    return r.code if isinstance(r, brotli_amd.BrotliError) else r


def _single(data):
    try:
        return brotli_amd.brotliDecode(data)
    except brotli_amd.BrotliError as e:
        return e.code


def test_big_build_single_streams():
    wrong = [name for name, data, exp in _cases() if _single(data) != exp]
    assert not wrong, wrong


def test_big_build_small_batches():
    cases, cus = _cases(), _cus()
    for i in range(0, len(cases), cus):
        chunk = cases[i:i + cus]
        outs = brotli_amd.decode_batch([c[1] for c in chunk])
        wrong = [name for (name, _, exp), got in zip(chunk, outs) if _got(got) != exp]
        assert not wrong, wrong


def test_root_window_stream_reaches_its_last_trees():
    """256 literal trees of 256 entries: tree 255's root is entry 65,536 and the command and
    distance roots lie beyond it.  Tables of 65,537..68,096 entries once went to LDS in the
    one-per-CU build, their roots cut to 16 bits: wrong bytes here, error -9 on placed_68096."""
    name, data, exp = next(c for c in _cases() if c[0] == 'lit256')
    assert _single(data) == exp
    name, data, exp = next(c for c in _cases() if c[0] == 'placed_68096')
    assert _single(data) == exp


def test_batch_build_mixed_placements():
    picked = _large_batch()
    names = {c[0] for c in picked}
    assert {'placed_12224', 'placed_12225', 'placed_30000', 'transitions', 'many_types', 'lit256'} <= names
    outs = brotli_amd.decode_batch([c[1] for c in picked])
    wrong = [name for (name, _, exp), got in zip(picked, outs) if _got(got) != exp]
    assert not wrong, wrong


def test_batch_build_device_context_exact_slots():
    import torch
    picked = _large_batch()
    dev = torch.device('cuda', 0)
    ioff, ooff = [0], [0]
    for _, data, exp in picked:
        ioff.append(ioff[-1] + len(data))
        ooff.append(ooff[-1] + len(exp))
    src = torch.frombuffer(bytearray(b''.join(c[1] for c in picked)), dtype=torch.uint8).to(dev)
    out = torch.zeros(ooff[-1] + 64, dtype=torch.uint8, device=dev)
    ctx = brotli_amd.DeviceContext(0)
    sizes, status = ctx.decode(src.data_ptr(), ioff, out.data_ptr(), ooff)
    assert status == [0] * len(picked)
    assert sizes == [len(c[2]) for c in picked]
    host = out.cpu().numpy().tobytes()
    for k, (name, _, exp) in enumerate(picked):
        assert host[ooff[k]:ooff[k + 1]] == exp, name
    assert host[ooff[-1]:] == bytes(64)


def test_transitions_between_placements_in_one_stream():
    """LDS tables, raw, HBM tables, metadata, LDS, raw, metadata, HBM in the batch build only, LDS:
    the 16-bit tables and the roots are re-established by every metablock"""
    name, data, exp = next(c for c in _cases() if c[0] == 'transitions')
    assert _single(data) == exp
    picked = _large_batch()
    outs = brotli_amd.decode_batch([c[1] for c in picked])
    hits = [k for k, c in enumerate(picked) if c[0] == 'transitions']
    assert hits
    for k in hits:
        assert _got(outs[k]) == exp


ERROR_STREAMS = ['placed_12224', 'placed_12225', 'placed_30000', 'lit256', 'placed_90000', 'transitions']


def _corrupted(name):
    """40 truncations and 40 single-bit flips of one stream, with the oracle's verdicts; half the
    flips anywhere (mostly the header of a many-tree stream), half in the last 40 % (commands)"""
    key = 'bad_' + name
    if key not in _cache:
        data = next(c[1] for c in _cases() if c[0] == name)
        rng = random.Random(len(name) * 131 + len(data))
        bad = [data[:rng.randrange(len(data))] for _ in range(40)]
        for k in range(40):
            bit = rng.randrange(8 * len(data) * 6 // 10 if k >= 20 else 0, 8 * len(data))
            b = bytearray(data)
            b[bit >> 3] ^= 1 << (bit & 7)
            bad.append(bytes(b))
        _cache[key] = [(name, d, _oracle.decode(d)) for d in bad]
    return _cache[key]


@pytest.mark.parametrize('name', ERROR_STREAMS)
def test_corrupted_streams_match_oracle(name):
    """the oracle's bytes or exactly the oracle's error code, on each placement"""
    for k, (_, data, exp) in enumerate(_corrupted(name)):
        assert _single(data) == exp, (name, k)


def test_corrupted_streams_in_the_batch_build():
    """the same corrupted streams between intact neighbours, more streams than CUs"""
    bad = [c for name in ERROR_STREAMS for c in _corrupted(name)]
    picked = _large_batch(extra=bad)
    outs = brotli_amd.decode_batch([c[1] for c in picked])
    wrong = [(k, c[0]) for k, (c, got) in enumerate(zip(picked, outs)) if _got(got) != c[2]]
    assert not wrong, wrong[:10]
    assert sum(1 for c in picked if isinstance(c[2], int)) >= 100
