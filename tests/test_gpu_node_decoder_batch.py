"""brotliDecoderUpdateBatch / brotliDecoderFinishBatch of the Node-API drop-in
(brotli-lib_amd/node), by tests/node/decoder_batch_test.js on the GPU: golden vectors in
lock-step chunks equal their plain files, and a corrupt stream in one slot gives the error
BrotliDecoder.update() throws, with the oracle's code, while the other slots decode."""
import base64
import json
import os
import re
import shutil
import subprocess

import pytest

import _inputs
import _oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_decoder_batch():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    with open(os.path.join(_inputs.GOLDEN, 'decode_errors.json')) as f:
        cases = json.load(f)['cases']
    # the longest corruption with a recorded decoder error (2,061 bytes: three of the test's chunks)
    case = max((c for c in cases if c.get('error', '').startswith('Brotli error code') and not c.get('hang')),
               key=lambda c: len(c['in_b64']))
    assert len(base64.b64decode(case['in_b64'])) > 2048
    code = _oracle.decode(base64.b64decode(case['in_b64']), -1)
    assert isinstance(code, int) and code == int(re.search(r'-\d+', case['error']).group())
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'decoder_batch_test.js'), case['in_b64'], str(code)],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
