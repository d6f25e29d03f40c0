"""Eight pieces a wave in the parse (dp_kernel<8>, enc_parse.hip: eight lanes a piece, one
price table and one literal-cost table a wave): the bytes of every stream must stay what they
were.  tests/golden/dp_ks8_digests.json holds each stream's size and SHA-256 as the commit
before that build encoded it (scripts/make_dp_ks8_digests.py; inputs and which build each case
reaches: tests/_dp_ks8_cases.py).  Every case: the bytes hash to the recorded digests, the HIP
decoder returns the inputs, the oracle decodes a handful, and a named subset equals its
single-stream encode, which takes the one-piece build -- another build in the same run.
"""
import json
import os

import pytest

import _dp_ks8_cases as cases
import _oracle
import brotli_amd

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp_ks8_digests.json')) as f:
    GOLDEN = json.load(f)['cases']

_enc = {}
_launched = {}   # case -> the parse's launches of its encode call, by pieces a wave


def _encoded(name):
    if name not in _enc:
        before = brotli_amd.debug_dp_launches()
        _enc[name] = cases.encode(name)
        after = brotli_amd.debug_dp_launches()
        _launched[name] = {ks: after[ks] - before[ks] for ks in after}
    return _enc[name]


@pytest.mark.parametrize('name', cases.CASES)
def test_the_case_reaches_the_build_it_is_named_for(name):
    """by what the library launched during the case's encode call: one eight-piece launch per
    encode lane (its second pass), none for the batch a stream short of the threshold -- and the
    piece counts of tests/_dp_ks8_cases.py say the same"""
    _encoded(name)
    got, lanes = _launched[name], cases.lanes(name)
    print(name, 'launches by pieces a wave', got, 'pieces a lane', lanes)
    if name == 'below_threshold':
        assert got[8] == 0 and got[2] >= 1, got
        assert lanes == [cases.THRESHOLD - 64]
    else:
        assert got[8] == len(lanes), (got, lanes)
        assert min(lanes) >= cases.THRESHOLD, lanes
    assert len(lanes) == {'two_lanes': 2, 'mib': 2}.get(name, 1)


def test_the_threshold_cases_stand_at_the_threshold():
    assert cases.lanes('at_threshold') == [cases.THRESHOLD]
    # one stream fewer in 'mib' and a lane falls below the threshold
    assert (cases.MIB_COUNT // 2 - 1) * cases.pieces(cases.MIB_LEN) < cases.THRESHOLD


@pytest.mark.parametrize('name', cases.CASES)
def test_bytes_are_the_recorded_ones_and_decode(name):
    bufs, got = cases.buffers(name), _encoded(name)
    assert len(got) == len(bufs) == len(GOLDEN[name])
    d = cases.digest(got)
    bad = [k for k in range(len(got)) if d[k] != GOLDEN[name][k]]
    back = cases.mib_device_roundtrip() if name == 'mib' else brotli_amd.decode_batch(got)
    print('%s: %d streams, %d -> %d bytes, %d differ %s%s' % (name, len(got), sum(map(len, bufs)), sum(map(len, got)), len(bad), bad[:40],
                                                             ', device round trip %s' % back if name == 'mib' else ''))
    assert not bad, 'streams %s: %s, recorded %s' % (bad[:8], [d[k] for k in bad[:8]], [GOLDEN[name][k] for k in bad[:8]])
    if name == 'mib':
        assert back
    else:
        wrong = [k for k in range(len(got)) if back[k] != bufs[k]]
        assert not wrong, 'HIP decoder, streams %s' % wrong[:8]
    for k in cases.ORACLE[name]:
        assert _oracle.decode(got[k], len(bufs[k])) == bufs[k], 'oracle, stream %d' % k


@pytest.mark.parametrize('name', cases.CASES)
def test_streams_equal_their_solo_encodes(name):
    """a stream parses the same in any batch and in any build of the parse"""
    bufs, got = cases.buffers(name), _encoded(name)
    for k in cases.SOLO[name]:
        assert brotli_amd.brotliEncode(bufs[k], cases.OPTS) == got[k], 'stream %d' % k
