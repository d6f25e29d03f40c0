"""The parse's step (dp_kernel, enc_parse.hip) reads its tables ahead of the node it waits
for; the bytes of every stream must stay what they were.  tests/golden/dp_chain_digests.json
holds each stream's size and SHA-256 as the build before that change encoded it
(scripts/make_dp_chain_digests.py; inputs: tests/_dp_chain_cases.py, which also says which
build of the kernel each case reaches and why).  Every case: the bytes hash to the recorded
digest, and the oracle decodes them to the input.
"""
import json
import os

import pytest

import _dp_chain_cases as cases
import _oracle
import brotli_amd

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp_chain_digests.json')) as f:
    GOLDEN = json.load(f)['cases']

_enc = {}


def _encoded(name):
    if name not in _enc:
        _enc[name] = cases.encode(name)
    return _enc[name]


@pytest.mark.parametrize('name', list(cases.CASES))
def test_bytes_are_the_recorded_ones_and_decode(name):
    bufs, got = cases.buffers(name), _encoded(name)
    assert len(got) == len(bufs) == len(GOLDEN[name])
    d = cases.digest(got)
    bad = [k for k in range(len(got)) if d[k] != GOLDEN[name][k]]
    print('%s: %d streams, %d -> %d bytes, %d differ' % (name, len(got), sum(map(len, bufs)), sum(map(len, got)), len(bad)))
    assert not bad, 'streams %s: %s, recorded %s' % (bad[:8], [d[k] for k in bad[:8]], [GOLDEN[name][k] for k in bad[:8]])
    dic = cases.options(name).get('customDictionary')
    for k, (s, b) in enumerate(zip(got, bufs)):
        assert _oracle.decode(s, len(b), dic) == b, 'stream %d' % k


def test_ks4_streams_equal_their_solo_encodes():
    """a stream parses the same in any batch: the first and last streams of the four-segment
    batch and the two at its lane boundary, each encoded alone (one-segment build)"""
    bufs, got = cases.buffers('ks4'), _encoded('ks4')
    for k in cases.KS4_SOLO:
        assert brotli_amd.brotliEncode(bufs[k], cases.options('ks4')) == got[k], 'stream %d' % k
