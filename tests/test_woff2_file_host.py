"""The WOFF2 container without a GPU: the parser and the serial assembly of
brotli-lib_amd/csrc/woff2_file.h, built as host code with AddressSanitizer and UBSan into a
stand-alone program (tests/woff2_file_host_main.cpp), turn every golden file and its
oracle-decoded stream into the golden sfnt, reject every item of the rejection list, take
damaged files without a report or a broken plan, and agree with the Python assembler that the
GPU test measures the kernels against."""
import hashlib
import os
import shutil
import struct
import subprocess
import sys

import pytest

import _oracle
import _woff2_file as wf
import _woff2_reconstruct as w2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, wf.HERE)

FUZZ_SEED = 20240611
FUZZ_DOUBLES = 6000   # random double edits per synthetic file, beside the structured damage


def test_goldens_are_fonttools_output():
    """the generator gives the committed JSON and binary fixtures again"""
    pytest.importorskip('fontTools')
    import make_file_golden
    out, files = make_file_golden.generate()
    assert out == wf.golden()
    assert sorted(files) == sorted(fx['file'] for fx in out['bench'].values())
    for name, data in files.items():
        with open(os.path.join(wf.HERE, name), 'rb') as f:
            assert f.read() == data, name


def test_known_tags_are_fonttools():
    pytest.importorskip('fontTools')
    from fontTools.ttLib.woff2 import woff2KnownTags
    assert tuple(t.encode('latin-1') for t in woff2KnownTags) == wf.KNOWN_TAGS


def test_fixtures_cover_both_transform_sets_and_stay_small():
    g = wf.golden()
    assert sorted(g['synthetic']) == ['synthetic', 'synthetic-hmtx']
    assert sorted(g['bench']) == ['enc-otf', 'enc-ttf', 'enc-ttf-hmtx', 'enc-var-ttf', 'enc-var-ttf-hmtx']
    for name, data, _, _, _ in wf.golden_files():
        _, ent, _ = wf.parse(data)
        state = {e[0]: wf.is_transformed(e[0], e[1]) for e in ent}
        assert state.get(b'hmtx', False) == name.endswith('-hmtx'), name
        assert state.get(b'glyf', False) == (name != 'enc-otf'), name
        assert len(data) < 512 * 1024
    assert os.path.getsize(os.path.join(wf.HERE, 'file_golden.json')) < 128 * 1024


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_file') / 'woff2_file_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_file_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _assemble(exe, tmp_path, pairs):
    """[(return code, sfnt)] of host_assemble over [(file, stream)]"""
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        for file, stream in pairs:
            f.write(w2.record(file) + w2.record(stream))
    assert _run(exe, 'assemble', src, dst).strip() == 'assembled %d' % len(pairs)
    with open(dst, 'rb') as f:
        b = f.read()
    out, at = [], 0
    while at < len(b):
        assert struct.unpack('<L', b[at:at + 4])[0] == 4
        rc = struct.unpack('<l', b[at + 4:at + 8])[0]
        n = struct.unpack('<L', b[at + 8:at + 12])[0]
        out.append((rc, b[at + 12:at + 12 + n]))
        at += 12 + n
    assert len(out) == len(pairs)
    return out


def _stream_of(file):
    return _oracle.decode(wf.parse(file)[2])


def test_host_assembly_matches_the_goldens(driver, tmp_path):
    gold = wf.golden_files()
    assert len(gold) == 7
    got = _assemble(driver, tmp_path, [(data, _stream_of(data)) for _, data, _, _, _ in gold])
    for (name, _, sfnt, size, sha), (rc, out) in zip(gold, got):
        assert rc == 0, name
        assert len(out) == size and hashlib.sha256(out).hexdigest() == sha, name
        if sfnt is not None:
            assert out == sfnt, name


def test_host_parser_rejects_the_list(driver, tmp_path):
    cases = wf.rejected_files(_oracle.decode)
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(1, 14))
    got = _assemble(driver, tmp_path, [(file, stream) for _, file, stream, _ in cases])
    for (name, _, _, _), (rc, out) in zip(cases, got):
        assert rc == -1 and out == b'', name


def test_host_parser_survives_damaged_files(driver, tmp_path):
    """Every truncation, every bit of the header fields a reader acts on and of the directory,
    every length field set to some 130 values, malformed UIntBase128s, and FUZZ_DOUBLES random
    double edits, of both synthetic files: 24,519 damaged files when this was written, 515
    (2.1 %) accepted -- a flag byte that names another unused tag, a transformed table's
    origLength (a hint), a smaller totalCompressedSize (the program gets the stream apart).
    The program itself exits non-zero on a plan whose sources leave the stream or whose
    destinations overlap or leave the announced size."""
    src = str(tmp_path / 'in.bin')
    with open(src, 'wb') as f:
        for hm in (False, True):
            file = wf.synthetic_file(hm)
            f.write(w2.record(file) + w2.record(_stream_of(file)))
    out = _run(driver, 'fuzz', src, FUZZ_SEED, FUZZ_DOUBLES).split()
    assert out[0] == 'damaged' and out[2] == 'accepted' and out[4] == 'rejected'
    damaged, accepted, rejected = int(out[1]), int(out[3]), int(out[5])
    print('damaged %d accepted %d rejected %d' % (damaged, accepted, rejected))
    assert damaged >= 20000 and accepted + rejected == damaged
    assert accepted > 0 and 20 * accepted < damaged


def test_host_assembly_agrees_with_the_python_assembler(driver, tmp_path):
    """the kernel-alone cases of the GPU test, as files whose tables all have the null transform"""
    cases = wf.assemble_cases()
    pairs = []
    for _, flavor, tables, _ in cases:
        ent = [[tag, 0, len(data), None] for tag, data in tables]
        pairs.append((wf.write(flavor, ent, b''), b''.join(data for _, data in tables)))
    got = _assemble(driver, tmp_path, pairs)
    for (name, flavor, tables, _), (rc, out) in zip(cases, got):
        assert rc == 0, name
        assert out == wf.assemble(flavor, tables), name
