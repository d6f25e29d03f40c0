"""The planning of a batch of streaming decoder sessions (brotli-lib_amd/csrc/stream_batch.h:
which sessions enter a round, the gather offsets and their alignment, the move descriptors'
block assignment, the decode grid) in a stand-alone program under AddressSanitizer and UBSan
(tests/stream_batch_host_main.cpp).  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_planning_under_sanitizers(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path / 'stream_batch_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'stream_batch_host_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(' ok') == 3, r.stdout
