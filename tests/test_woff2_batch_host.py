"""The WOFF2 batch plan without a GPU: brotli-lib_amd/csrc/woff2_batch.h -- groups, stream slots,
the assembly launch's descriptors -- built as host code with AddressSanitizer and UBSan into a
stand-alone program (tests/woff2_batch_host_main.cpp) that plans calls of the golden files in
varied orders and under group budgets of 1 byte, one file's size and the default, checks the
plan's invariants itself (it exits non-zero on a broken one) and, with host_assemble as the
per-font worker and the kernels stated serially, gives the golden sfnts."""
import hashlib
import os
import random
import shutil
import struct
import subprocess

import pytest

import _oracle
import _woff2_file as wf
import _woff2_reconstruct as w2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_batch') / 'woff2_batch_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_batch_host_main.cpp'), '-o', exe], check=True)
    return exe


@pytest.fixture(scope='module')
def gold():
    """[(name, file, stream, sfnt or None, size, sha256)]: the streams decoded once"""
    out = [(name, data, _oracle.decode(wf.parse(data)[2]), sfnt, size, sha) for name, data, sfnt, size, sha in wf.golden_files()]
    assert len(out) == 7
    return out


def _plan(exe, tmp_path, pairs, budget):
    """([(code, sfnt)], {files, parsed, groups, fonts}) of one planned call over [(file, stream)]"""
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        for file, stream in pairs:
            f.write(w2.record(file) + w2.record(stream))
    r = subprocess.run([exe, 'plan', src, dst, str(budget)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    counts = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    with open(dst, 'rb') as f:
        b = f.read()
    out, at = [], 0
    while at < len(b):
        assert struct.unpack('<L', b[at:at + 4])[0] == 4
        rc = struct.unpack('<l', b[at + 4:at + 8])[0]
        n = struct.unpack('<L', b[at + 8:at + 12])[0]
        out.append((rc, b[at + 12:at + 12 + n]))
        at += 12 + n
    assert len(out) == len(pairs) == counts['files']
    return out, counts


def _orders(gold):
    n = len(gold)
    rng = random.Random(7)
    shuffled = list(range(n)) + [1, 4]   # two of them twice
    rng.shuffle(shuffled)
    return {'directory': list(range(n)), 'reversed': list(range(n))[::-1], 'shuffled-with-repeats': shuffled,
            'one': [3], 'small-last': [2, 3, 4, 5, 6, 0, 1]}


def _check(gold, order, got):
    for g, (rc, out) in zip(order, got):
        name, _, _, sfnt, size, sha = gold[g]
        assert rc == 0, name
        assert len(out) == size and hashlib.sha256(out).hexdigest() == sha, name
        if sfnt is not None:
            assert out == sfnt, name


@pytest.mark.parametrize('order', ['directory', 'reversed', 'shuffled-with-repeats', 'one', 'small-last'])
def test_planned_batches_give_the_goldens(driver, gold, tmp_path, order):
    idx = _orders(gold)[order]
    pairs = [(gold[g][1], gold[g][2]) for g in idx]
    lens = [len(gold[g][2]) for g in idx]
    one_file = sorted(lens)[len(lens) // 2]
    for budget in (1, one_file, 0):
        got, counts = _plan(driver, tmp_path, pairs, budget)
        _check(gold, idx, got)
        assert counts['parsed'] == counts['fonts'] == len(idx)
        # what the greedy cut gives, stated again here
        groups, room = 0, 0
        limit = budget or 512 << 20
        alone = False
        for n in lens:
            if groups == 0 or alone or n > limit or n > room:
                groups, room = groups + 1, limit
            room -= min(n, room)
            alone = n > limit
        assert counts['groups'] == groups, (budget, lens)
        if budget == 1:
            assert groups == len(idx)
        if budget == 0:
            assert groups == 1


def test_unparsable_and_rejected_files_between_the_goldens(driver, gold, tmp_path):
    """files that do not parse take no place in any group; one that parses around a stream of
    another size, or around tables the reconstruction rejects, drops out of its group's launch"""
    bad = wf.rejected_files(_oracle.decode)
    pairs, want = [], []
    for i, (name, file, stream, edited) in enumerate(bad):
        pairs.append((file, stream))
        want.append(None)
        g = gold[i % len(gold)]
        pairs.append((g[1], g[2]))
        want.append(i % len(gold))
    unparsable = sum(1 for name, _, _, edited in bad if not edited and int(name.split('-')[0]) <= 11)
    for budget in (1, len(gold[0][2]), 0):
        got, counts = _plan(driver, tmp_path, pairs, budget)
        assert counts['parsed'] == len(pairs) - unparsable
        assert counts['fonts'] == len(bad)   # the goldens and nothing else
        for w, (rc, out) in zip(want, got):
            if w is None:
                assert rc == -1 and out == b''
            else:
                _check(gold, [w], [(rc, out)])


def test_plan_agrees_with_the_python_assembler(driver, tmp_path):
    """the kernel-alone cases of the GPU test in one call, as files whose tables all have the null
    transform: fonts of many table counts and lengths side by side in one launch"""
    cases = wf.assemble_cases()
    pairs = []
    for _, flavor, tables, _ in cases:
        ent = [[tag, 0, len(data), None] for tag, data in tables]
        pairs.append((wf.write(flavor, ent, b''), b''.join(data for _, data in tables)))
    for budget in (0, 64):
        got, counts = _plan(driver, tmp_path, pairs, budget)
        assert counts['fonts'] == len(cases)
        for (name, flavor, tables, _), (rc, out) in zip(cases, got):
            assert rc == 0, name
            assert out == wf.assemble(flavor, tables), name
