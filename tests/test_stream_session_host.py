"""The streaming decoder session's host arithmetic (brotli-lib_amd/csrc/stream_session.h: the
first checkpoint, which pending input a resume still reads, rebasing when input is dropped
and when the history moves down, buffer sizing) in a stand-alone program under
AddressSanitizer and UBSan (tests/stream_session_host_main.cpp).  No GPU, nothing loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_session_arithmetic_under_sanitizers(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path / 'stream_session_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'stream_session_host_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count('lgwin') == 3, r.stdout
