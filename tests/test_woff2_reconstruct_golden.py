"""The inverse WOFF2 transforms without a GPU: the goldens are fontTools' output, and the
walker the GPU kernels compile (brotli-lib_amd/csrc/woff2_inv.h), built as host code with
AddressSanitizer and UBSan into a stand-alone program (tests/woff2_inv_host_main.cpp),
reconstructs every fixture byte for byte and takes damaged tables without a report."""
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

import _oracle  # noqa: F401  (make_golden.fonts decodes a bench font with it)
import _woff2_reconstruct as w2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, w2.HERE)

FUZZ_SEED = 20240607
FUZZ_EDITS = 11000   # single-byte edits per synthetic table; two tables, plus the structured damage


def test_goldens_are_fonttools_output():
    pytest.importorskip('fontTools')
    import make_reconstruct_golden
    assert make_reconstruct_golden.generate() == w2.golden()


def test_all_empty_font_is_one_zero_byte_in_fonttools():
    pytest.importorskip('fontTools')
    from fontTools.ttLib import TTFont, newTable
    from fontTools.ttLib.woff2 import WOFF2GlyfTable, WOFF2LocaTable
    t, glyf, loca = w2.all_empty()
    font = TTFont()
    font.recalcBBoxes = False
    font.setGlyphOrder(['g%d' % i for i in range(5)])
    font['head'] = newTable('head')
    g = WOFF2GlyfTable()
    g.reconstruct(t, font)
    g.padding = 4
    font['loca'] = WOFF2LocaTable()
    font['glyf'] = g
    assert g.compile(font) == glyf
    assert font['loca'].compile(font) == loca


def test_synthetic_fixture_is_small_and_has_both_loca_formats():
    fx = w2.synthetic()
    assert sorted(fx) == ['fmt0', 'fmt1']
    for k, f in fx.items():
        assert f['tglyf'][6:8] == (b'\0\0' if k == 'fmt0' else b'\0\1')
        assert len(f['tglyf']) < 16384 and f['num_glyphs'] < 48
        assert len(f['loca']) == (f['num_glyphs'] + 1) * (2 if k == 'fmt0' else 4)
    assert os.path.getsize(os.path.join(w2.HERE, 'reconstruct_golden.json')) < 128 * 1024


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_inv') / 'woff2_inv_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_inv_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _fixture_file(path):
    rec = []
    for _, f in sorted(w2.synthetic().items()):
        rec += [f['tglyf'], f['glyf'], f['loca'], f['thmtx'], f['hmtx'], f['num_glyphs'].to_bytes(4, 'little'),
                f['num_hmetrics'].to_bytes(4, 'little')]
    rec += list(w2.all_empty()) + [b'', b'', bytes(4), bytes(4)]
    with open(path, 'wb') as out:
        out.write(b''.join(w2.record(r) for r in rec))


def test_host_walker_matches_fixtures(driver, tmp_path):
    p = str(tmp_path / 'fixtures.bin')
    _fixture_file(p)
    assert _run(driver, 'check', p).strip() == 'checked 3'


def test_host_walker_matches_bench_font_hashes(driver, tmp_path):
    """the bench fonts: their transformed tables need fontTools here (the GPU test makes them
    with the forward kernels); the driver's output is compared through a fixture file"""
    pytest.importorskip('fontTools')
    import make_golden
    import make_reconstruct_golden as gen
    gold = w2.golden()['bench']
    rec = []
    for name, ttf in make_golden.fonts():
        t = make_golden.transform(ttf)
        assert hashlib.sha256(t).hexdigest() == gold[name]['tglyf_sha256']
        glyf, loca, _ = gen.reconstruct(ttf, t)
        assert hashlib.sha256(glyf).hexdigest() == gold[name]['glyf_sha256']
        assert hashlib.sha256(loca).hexdigest() == gold[name]['loca_sha256']
        rec += [t, glyf, loca, b'', b'', bytes(4), bytes(4)]
    p = str(tmp_path / 'bench.bin')
    with open(p, 'wb') as out:
        out.write(b''.join(w2.record(r) for r in rec))
    assert _run(driver, 'check', p).strip() == 'checked 2'
    # 140 KB of glyphs under indexFormat 0: offsets that a 16-bit loca cannot hold
    p = str(tmp_path / 'short_loca.bin')
    with open(p, 'wb') as out:
        for r in (b'glyf', w2.with_short_loca(rec[0]), b'', b'', bytes(4), bytes(4)):
            out.write(w2.record(r))
    assert _run(driver, 'reject', p).strip() == 'rejected 1'


def test_host_walker_rejects_the_bad_inputs(driver, tmp_path):
    cases = w2.bad_inputs()
    assert len(cases) >= 12
    p = str(tmp_path / 'bad.bin')
    with open(p, 'wb') as out:
        for _, kind, table, fx in cases:
            hm = kind == 'hmtx'
            for r in (kind.encode(), table, fx['glyf'] if hm else b'', fx['loca'] if hm else b'',
                      fx['num_glyphs'].to_bytes(4, 'little'), fx['num_hmetrics'].to_bytes(4, 'little')):
                out.write(w2.record(r))
    assert _run(driver, 'reject', p).strip() == 'rejected %d' % len(cases)


def test_host_walker_survives_damaged_inputs(driver, tmp_path):
    """Single-byte edits, truncations (every length below 64, every stream boundary), header
    sizes moved by 1 and 255: each copy is rejected or reconstructs within the announced size;
    no sanitizer report, exit status 0.  The device code is the same text."""
    p = str(tmp_path / 'fixtures.bin')
    _fixture_file(p)
    out = _run(driver, 'fuzz', p, FUZZ_SEED, FUZZ_EDITS).split()
    assert out[0] == 'damaged' and out[2] == 'accepted' and out[4] == 'rejected'
    damaged, accepted, rejected = int(out[1]), int(out[3]), int(out[5])
    print('damaged %d accepted %d rejected %d' % (damaged, accepted, rejected))
    assert damaged >= 20000 and accepted + rejected == damaged
    # both outcomes occur: an edit inside the instructions is harmless, a cut stream is not
    assert accepted > 0 and rejected > 0
