"""The planning of the device-resident session calls (brotli-lib_amd/csrc/stream_batch.h: what a
slot delivers and goes on holding, when it launches and with which output limit, when it reports
MORE_OUTPUT, the copy launches' grids and their split) in a stand-alone program under
AddressSanitizer and UBSan (tests/stream_deliver_host_main.cpp).  No GPU, nothing loaded into
Python."""
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
    assert r.stdout.count(' ok') == 3, r.stdout
