"""The rounds of the session calls -- mib::stream_rounds, the product's own loop
(brotli-lib_amd/csrc/stream_rounds.h: admission, who launches and with which output limit, the
accounting of a launch, what a slot delivers and goes on holding, when it reports MORE_OUTPUT,
input compaction) over a model device, and the copy launches' grids and their split
(stream_batch.h) -- in a stand-alone program under AddressSanitizer and UBSan
(tests/stream_deliver_host_main.cpp).  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_delivery_planning_under_sanitizers(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path / 'stream_deliver_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'stream_deliver_host_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(' ok') == 7, r.stdout
