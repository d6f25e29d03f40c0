"""The backtrack's window walk on the vector side (backtrack_kernel, enc_parse.hip: the path
through a window by pointer doubling, commands stored by their copy nodes' lanes, pieces'
commands left where the walk wrote them, no memset of the choices): the bytes of every stream
must stay what they were.  tests/golden/backtrack_digests.json holds each stream's size and
SHA-256 as the commit before that change encoded it (scripts/make_backtrack_digests.py; inputs
and what each case exercises: tests/_backtrack_cases.py).  Every case: the bytes hash to the
recorded digests, the HIP decoder returns the inputs, the oracle decodes a handful; a batch
equals its streams' solo encodes; and calls that find an earlier call's choices under every
position still give the recorded bytes.
"""
import json
import os

import pytest

import _backtrack_cases as cases
import _oracle
import brotli_amd

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backtrack_digests.json')) as f:
    GOLDEN = json.load(f)['cases']

_enc = {}


def _encoded(name):
    if name not in _enc:
        _enc[name] = cases.encode(name)
    return _enc[name]


def test_the_fixture_has_every_case():
    assert sorted(GOLDEN) == sorted(cases.CASES)


@pytest.mark.parametrize('name', cases.CASES)
def test_bytes_are_the_recorded_ones_and_decode(name):
    bufs, got = cases.buffers(name), _encoded(name)
    assert len(got) == len(bufs) == len(GOLDEN[name])
    d = cases.digest(got)
    bad = [k for k in range(len(got)) if d[k] != GOLDEN[name][k]]
    print('%s: %d streams, %d -> %d bytes, %d differ %s' % (name, len(got), sum(map(len, bufs)), sum(map(len, got)), len(bad), bad[:40]))
    assert not bad, 'streams %s: %s, recorded %s' % (bad[:8], [d[k] for k in bad[:8]], [GOLDEN[name][k] for k in bad[:8]])
    back = brotli_amd.decode_batch(got)
    wrong = [k for k in range(len(got)) if back[k] != bufs[k]]
    assert not wrong, 'HIP decoder, streams %s' % wrong[:8]
    for k in cases.ORACLE.get(name, ()):
        assert _oracle.decode(got[k], len(bufs[k])) == bufs[k], 'oracle, stream %d' % k


def test_a_batch_equals_its_streams_solo_encodes():
    """'mixed' is every solo case's streams in one call (pieces of 1, 2 and 8 KiB side by side);
    'two_lanes' is cut into two encode lanes between streams 255 and 256"""
    solo = [s for n in cases.SOLO_CASES for s in _encoded(n)]
    mixed = _encoded('mixed')
    assert len(mixed) == len(solo)
    assert [k for k in range(len(solo)) if mixed[k] != solo[k]] == []
    bufs, got = cases.buffers('two_lanes'), _encoded('two_lanes')
    assert brotli_amd.decode_batch(got) == bufs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp_ks8_digests.json')) as f:
        assert cases.digest(got) == json.load(f)['cases']['two_lanes']   # (the same 512 streams, recorded there)
    for k in cases.TWO_LANES_SOLO:
        assert brotli_amd.brotliEncode(bufs[k], {'quality': 11}) == got[k], 'stream %d' % k
    assert _oracle.decode(got[255], len(bufs[255])) == bufs[255]


def test_stale_choices_of_the_call_before_change_nothing():
    """one context's workspace through five calls of the same positions: the long-run stream (its
    forced long copies leave their interiors unwritten), text of its length, and batches of both"""
    want_a, want_b = GOLDEN['long_run'][0], GOLDEN['long_run_twin'][0]
    calls = cases.stale_choices()
    got = [cases.digest(c) for c in calls]
    print([[d[0] for d in c] for c in got])
    assert got == [[want_a, want_b], [want_a], [want_b], [want_a], [want_a, want_b]]
    assert brotli_amd.decode_batch(calls[4]) == [cases.buffers('long_run')[0], cases.buffers('long_run_twin')[0]]
