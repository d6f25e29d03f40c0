"""The backtrack's window walk without a GPU: brotli-lib_amd/csrc/backtrack_window.h (the path
through a window of 64 nodes by pointer doubling, the copy nodes' ranks and literal counts from
its ballot -- the text backtrack_kernel runs on a wave) on arrays of 64, against the plain walk
node by node (tests/backtrack_window_host_main.cpp), run as a child process.  Built twice: plain
for the longest exhaustive run, and with AddressSanitizer and UBSan for a shorter one and the
random windows."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'backtrack_window_host_main.cpp')


def _build(tmp_path_factory, name, flags):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([gxx, '-std=c++17', *flags, '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'), SRC, '-o', exe],
                   check=True)
    return exe


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    return _build(tmp_path_factory, 'backtrack_window_host', ['-O3'])


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory, 'backtrack_window_host_san',
                  ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


def _start(exe, *args):
    return subprocess.Popen([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _checks(proc):
    out, err = proc.communicate(timeout=300)
    assert proc.returncode == 0 and not err, (out[-2000:], err[-4000:])
    last = out.splitlines()[-1]
    assert last.startswith('ok ')
    return int(last.split()[1])


def _run(exe, *args):
    return _checks(_start(exe, *args))


def _exhaustive_checks(full, small):
    """windows times entries of `exhaustive FULL SMALL`, all parts together"""
    n_full = 0
    for n in range(1, full + 1):
        pats = 1
        for x in range(n):
            pats *= n - x + 3   # 0 .. n - x + 1, and 64 beyond the end
        n_full += pats * n
    return n_full + sum(3 ** n * n for n in range(full + 1, small + 1))


PARTS = 4   # child processes side by side


def test_every_window_of_up_to_12_positions(plain, sanitized):
    """up to 6 positions: every length that behaves differently at each position; 7 to 12: every
    pattern of literals and copies of 2 and 3; every entry of each.  Under the sanitizers: up to 5
    and 8 positions"""
    procs = [_start(plain, 'exhaustive', 6, 12, part, PARTS) for part in range(PARTS)]
    san = _start(sanitized, 'exhaustive', 5, 8, 0, 1)
    assert sum(_checks(p) for p in procs) == _exhaustive_checks(6, 12)
    assert _checks(san) == _exhaustive_checks(5, 8)


@pytest.mark.parametrize('seed', (1, 20261))
def test_random_windows_of_64_positions(plain, sanitized, seed):
    """every nvalid and entry: drawn lengths up to the segment's limit, no copy, copies of 2 only,
    a copy leaving the window by exactly 0, 1 and 64 positions"""
    # per nvalid n: four kinds of window at n entries, and the leaving copy at each entry and (where
    # the window has room) two literals below it, by three amounts
    per_round = sum(4 * n + 3 * (n + max(n - 2, 0)) for n in range(1, 65))
    assert _run(plain, 'random', seed, 8) == 8 * per_round
    assert _run(sanitized, 'random', seed, 2) == 2 * per_round
