"""The WOFF2 writer's plan without a GPU: brotli-lib_amd/csrc/woff2_write.h, built as host code with
AddressSanitizer and UBSan into a stand-alone program (tests/woff2_write_host_main.cpp), gives
every golden file's directory, header and decompressed stream again from the file's source font
and the transformed tables cut out of the golden stream, rejects every item of the rejection
list, and takes damaged fonts without a report or a broken plan."""
import os
import shutil
import struct
import subprocess

import pytest

import _woff2_file as wf
import _woff2_reconstruct as w2
import _woff2_write as ww
from brotli_amd import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_write') / 'woff2_write_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_write_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _pack(exe, tmp_path, cases):
    """[(parse's answer, directory, header, stream)] over [(sfnt, transforms, tglyf, thmtx, compressed size)]"""
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        for sfnt, transforms, tglyf, thmtx, comp in cases:
            f.write(w2.record(sfnt) + w2.record(bytes([transforms])) + w2.record(tglyf) + w2.record(thmtx) +
                    w2.record(struct.pack('<L', comp)))
    assert _run(exe, 'pack', src, dst).strip() == 'packed %d' % len(cases)
    with open(dst, 'rb') as f:
        b = f.read()
    recs, at = [], 0
    while at < len(b):
        n = struct.unpack('<L', b[at:at + 4])[0]
        recs.append(b[at + 4:at + 4 + n])
        at += 4 + n
    assert len(recs) == 4 * len(cases)
    return [(struct.unpack('<l', recs[i])[0], recs[i + 1], recs[i + 2], recs[i + 3]) for i in range(0, len(recs), 4)]


def test_plan_gives_the_goldens_again(driver, tmp_path):
    gold = ww.golden_cases()
    assert len(gold) == 7
    cases = []
    for name, src, data, transforms, _, _ in gold:
        ent, stream = ww.golden_stream(data)
        parts = wf.cut(ent, stream)
        state = {e[0]: wf.is_transformed(e[0], e[1]) for e in ent}
        assert state.get(b'hmtx', False) == bool(transforms & ww.HMTX), name
        cases.append((src, transforms, parts[b'glyf'] if state.get(b'glyf') else b'', parts[b'hmtx'] if state.get(b'hmtx') else b'',
                      struct.unpack('>L', data[20:24])[0]))
    for (name, src, data, _, _, _), (rc, directory, header, stream) in zip(gold, _pack(driver, tmp_path, cases)):
        assert rc == 0, name
        assert directory == ww.directory_bytes(data), name
        assert header == data[:48], name
        ent, want = ww.golden_stream(data)
        assert stream == ww.zero_head(ent, want), name


def test_plan_of_the_hand_built_fonts(driver, tmp_path):
    """the copy kernel's cases of the GPU test: directory and stream as the Python statement has them"""
    cases = ww.pack_cases()
    got = _pack(driver, tmp_path, [(font, 3, b'', b'', 5) for _, font, _ in cases])
    for (name, font, tables), (rc, directory, header, stream) in zip(cases, got):
        assert rc == 0, name
        ent, want = ww.expected_entries_and_stream(tables)
        flavor = struct.unpack('>L', font[:4])[0]
        assert header + directory == ww.expected_prefix(flavor, ent, tables, 5), name
        assert stream == want, name


def test_plan_rejects_the_list(driver, tmp_path):
    cases = ww.rejected_fonts()
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(1, 9))
    for transforms in (0, 3):
        got = _pack(driver, tmp_path, [(font, transforms, b'', b'', 0) for _, font in cases])
        for (name, _), (rc, directory, header, stream) in zip(cases, got):
            assert rc == int(name.split('-')[0]), name
            assert directory == header == stream == b'', name


def test_plan_rejects_what_the_glyf_transform_needs(driver, tmp_path):
    ttf = wf.font_with_metrics(datagen.glyf_font(41, 60))
    cases = ww.glyf_needs_fonts(ttf)
    got = _pack(driver, tmp_path, [(font, 3, b'', b'', 0) for _, font in cases])
    for (name, _), (rc, _, _, _) in zip(cases, got):
        assert rc == 9, name
    # with the transform off the same fonts are stored as they are
    got = _pack(driver, tmp_path, [(font, 0, b'', b'', 0) for _, font in cases])
    assert [g[0] for g in got] == [0] * len(cases)


def test_plan_survives_damaged_fonts(driver, tmp_path):
    """Every truncation up to the directory's end, every bit of the offset table and the directory,
    and every offset and length field set to some 56 values, of a synthetic TrueType font with
    metrics and a hand-built font with a DSIG and an unknown tag.  The program itself exits
    non-zero on a plan whose source ranges leave the input or whose stream pieces overlap or
    leave stream_len, and runs host_pack over every accepted plan under the sanitizers."""
    src = str(tmp_path / 'in.bin')
    hand = [c for c in ww.pack_cases() if c[0] in ('dsig', 'unknown-tags')]
    with open(src, 'wb') as f:
        f.write(w2.record(wf.font_with_metrics(datagen.glyf_font(41, 60))))
        for _, font, _ in hand:
            f.write(w2.record(font))
    out = _run(driver, 'fuzz', src).split()
    assert out[0] == 'damaged' and out[2] == 'accepted' and out[4] == 'rejected' and out[6] == 'why'
    damaged, accepted, rejected = int(out[1]), int(out[3]), int(out[5])
    print(' '.join(out))
    assert damaged >= 3000 and accepted + rejected == damaged
    assert accepted > 0 and rejected > damaged // 4
