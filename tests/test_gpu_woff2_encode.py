"""woff2_encode / woff2_encode_batch on the GPU (brotli-lib_amd/csrc/woff2_write.hip, woff2_write.h):
the files written for the golden files' source fonts say what fontTools' files say in every byte
but the Brotli stream, and decode to the golden sfnts; a font that is not normalised round-trips
through woff2_decode; the options choose the transforms; the copy kernel keeps every byte at
every alignment; what the list rejects is rejected; a batch gives per slot what the solo call
gives, however it is cut into groups."""
import hashlib
import os
import shutil
import struct
import subprocess
import sys

import pytest

import _woff2_file as wf
import _woff2_write as ww
import brotli_amd
from brotli_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q5 = {'quality': 5, 'lgwin': 18}   # (where the Brotli bits are not what is looked at)


@pytest.fixture(scope='module')
def ttf():
    return wf.font_with_metrics(datagen.glyf_font(41, 800))


def _solo(font, options=None):
    try:
        return brotli_amd.woff2_encode(font, options)
    except brotli_amd.BrotliError as e:
        return e.code


def _decode(file):
    try:
        return brotli_amd.woff2_decode(file)
    except brotli_amd.BrotliError as e:
        return e.code


def _stream(file):
    return brotli_amd.brotliDecode(wf.parse(file)[2])


def _check_file(file, flavor, ent, tables):
    """header, directory and padding of a file, given its entries"""
    comp = struct.unpack('>L', file[20:24])[0]
    prefix = ww.expected_prefix(flavor, ent, tables, comp)
    assert file[:len(prefix)] == prefix
    assert len(file) == (len(prefix) + comp + 3) & ~3 and not any(file[len(prefix) + comp:])


def test_goldens():
    for name, src, gold, transforms, size, sha in ww.golden_cases():
        file = brotli_amd.woff2_encode(src, ww.options(transforms))
        flavor, ent, _ = wf.parse(file)
        gflavor, gent, _ = wf.parse(gold)
        assert (flavor, ent) == (gflavor, gent), name
        assert file[16:20] == gold[16:20], name   # totalSfntSize
        assert file[24:48] == gold[24:48] and file[12:16] == gold[12:16], name
        at = len(ww.directory_bytes(gold)) + 48
        assert file[48:at] == gold[48:at], name
        assert len(file) % 4 == 0 and len(file) - at - struct.unpack('>L', file[20:24])[0] < 4, name
        gent, gstream = ww.golden_stream(gold)
        assert _stream(file) == ww.zero_head(gent, gstream), name
        out = brotli_amd.woff2_decode(file)
        assert len(out) == size and hashlib.sha256(out).hexdigest() == sha, name


def _want_transformed(ttf, tables=None):
    t = dict(tables or wf.sfnt_tables(ttf))
    t[b'glyf'], t[b'loca'] = brotli_amd.woff2_reconstruct_glyf(brotli_amd.woff2_transform_glyf(ttf))
    h = t[b'head']
    t[b'head'] = h[:16] + bytes([h[16] | 8]) + h[17:]
    return wf.assemble(struct.unpack('>L', ttf[:4])[0], sorted(t.items()))


def test_a_font_that_is_not_normalised(ttf):
    t = wf.sfnt_tables(ttf)
    file = brotli_amd.woff2_encode(ttf)
    _, ent, _ = wf.parse(file)
    assert [e[0] for e in ent] == sorted(t)
    ver = {e[0]: e[1] for e in ent}
    assert ver[b'hmtx'] == 1 and ver[b'glyf'] == 0 and ver[b'loca'] == 0
    assert {e[0]: e[2] for e in ent} == {tag: len(data) for tag, data in t.items()}   # origLength: the input's
    want = _want_transformed(ttf)
    assert brotli_amd.woff2_decode(file) == want
    parts = wf.cut(ent, _stream(file))
    assert parts[b'glyf'] == brotli_amd.woff2_transform_glyf(ttf)
    assert parts[b'hmtx'] == brotli_amd.woff2_transform_hmtx(ttf)
    assert parts[b'loca'] == b''


def test_options(ttf):
    t = wf.sfnt_tables(ttf)
    flavor = struct.unpack('>L', ttf[:4])[0]
    # both transforms off
    file = brotli_amd.woff2_encode(ttf, dict(Q5, transformGlyf=False, transformHmtx=False))
    ent = wf.parse(file)[1]
    assert {e[0]: e[1] for e in ent} == {tag: (3 if tag in (b'glyf', b'loca') else 0) for tag in t}
    assert all(e[3] is None for e in ent)
    assert brotli_amd.woff2_decode(file) == wf.assemble(flavor, sorted(t.items()))
    want_ent, want_stream = ww.expected_entries_and_stream(list(t.items()))
    assert ent == want_ent and _stream(file) == want_stream
    _check_file(file, flavor, ent, list(t.items()))
    # glyf off, hmtx asked for: hmtx needs glyf
    file = brotli_amd.woff2_encode(ttf, dict(Q5, transformGlyf=False))
    assert wf.parse(file)[1] == want_ent
    # hmtx off only
    file = brotli_amd.woff2_encode(ttf, dict(Q5, transformHmtx=False))
    ver = {e[0]: e[1] for e in wf.parse(file)[1]}
    assert ver[b'hmtx'] == 0 and ver[b'glyf'] == 0 and ver[b'loca'] == 0
    assert brotli_amd.woff2_decode(file) == _want_transformed(ttf)
    # an hmtx with one trailing byte is stored as it is
    u = dict(t)
    u[b'hmtx'] = t[b'hmtx'] + b'\x07'
    odd = wf.assemble(flavor, sorted(u.items()))
    file = brotli_amd.woff2_encode(odd, Q5)
    ent = wf.parse(file)[1]
    ver = {e[0]: e[1] for e in ent}
    assert ver[b'hmtx'] == 0 and ver[b'glyf'] == 0
    assert wf.cut(ent, _stream(file))[b'hmtx'] == u[b'hmtx']
    assert brotli_amd.woff2_decode(file) == _want_transformed(odd)
    # side bearings: one array off xMin keeps the transform, both store the table as it is
    sys.path.insert(0, wf.HERE)
    import make_golden
    variants = dict(make_golden.hmtx_variants(ttf))
    assert sorted(variants) == ['asis', 'both', 'mono', 'prop']
    for name, font in variants.items():
        file = brotli_amd.woff2_encode(font, Q5)
        ent = wf.parse(file)[1]
        ver = {e[0]: e[1] for e in ent}
        assert ver[b'hmtx'] == (0 if name == 'both' else 1), name
        got = wf.cut(ent, _stream(file))[b'hmtx']
        assert got == (wf.sfnt_tables(font)[b'hmtx'] if name == 'both' else brotli_amd.woff2_transform_hmtx(font)), name
        assert brotli_amd.woff2_decode(file) == _want_transformed(font), name
    # quality and window
    want = _want_transformed(ttf)
    for q, w in ((5, 18), (0, 10)):
        file = brotli_amd.woff2_encode(ttf, {'quality': q, 'lgwin': w})
        assert brotli_amd.woff2_decode(file) == want, (q, w)
    # an unknown transforms bit
    with pytest.raises(brotli_amd.BrotliError) as e:
        brotli_amd.woff2_encode(ttf, {'transforms': 4})
    assert e.value.code == wf.MIB_E_INVALID_ARG
    with pytest.raises(brotli_amd.BrotliError) as e:
        brotli_amd.woff2_encode_batch([ttf, ttf], {'transforms': 0x80000001})
    assert e.value.code == wf.MIB_E_INVALID_ARG


def test_the_pack_kernels_edges():
    cases = ww.pack_cases()
    files = brotli_amd.woff2_encode_batch([font for _, font, _ in cases], Q5)
    for (name, font, tables), file in zip(cases, files):
        assert isinstance(file, bytes), (name, file)
        flavor = struct.unpack('>L', font[:4])[0]
        ent, want = ww.expected_entries_and_stream(tables)
        assert wf.parse(file)[1] == ent, name
        _check_file(file, flavor, ent, tables)
        assert b'DSIG' not in [e[0] for e in ent] and b'DSIG' not in file[:len(file) - struct.unpack('>L', file[20:24])[0] - 3], name
        assert _stream(file) == want, name
        kept = [(tag, data) for tag, data in sorted(tables) if tag != b'DSIG']
        assert brotli_amd.woff2_decode(file) == wf.assemble(flavor, kept), name
    # ... and each alone says the same in every byte but the Brotli stream's
    for (name, font, tables), file in list(zip(cases, files))[::7]:
        solo = brotli_amd.woff2_encode(font, Q5)
        assert wf.parse(solo)[:2] == wf.parse(file)[:2] and _stream(solo) == _stream(file), name


def test_rejections(ttf):
    for name, font in ww.rejected_fonts():
        for options in (None, {'transformGlyf': False}):
            assert _solo(font, options) == wf.MIB_E_INVALID_ARG, name
    for name, font in ww.glyf_needs_fonts(ttf):
        assert _solo(font) == wf.MIB_E_INVALID_ARG, name
        assert isinstance(_solo(font, dict(Q5, transformGlyf=False)), bytes), name   # stored as they are
    bad = ww.malformed_glyph_font(ttf)
    assert _solo(bad) == wf.MIB_E_INVALID_ARG
    assert isinstance(_solo(bad, dict(Q5, transformGlyf=False)), bytes)


def test_batch_in_groups(ttf):
    gold = ww.golden_cases()
    syn, syn_hm, otf = gold[0][1], gold[1][1], gold[2][1]
    assert gold[2][0] == 'enc-otf'
    rejected = ww.rejected_fonts()[4][1]
    bad_glyph = ww.malformed_glyph_font(ttf)
    fonts = [syn, ttf, rejected, otf, ttf, bad_glyph, syn_hm, b'', syn, gold[3][1], bad_glyph, ttf]
    solo = [_solo(f, Q5) for f in fonts]
    assert [s for s in solo if not isinstance(s, bytes)] == [wf.MIB_E_INVALID_ARG] * 4
    results = {}
    try:
        for budget in (0, 400 * 1024, 1):   # one group; four; a font each
            brotli_amd.force_woff2_group_bytes(budget)
            results[budget] = brotli_amd.woff2_encode_batch(fonts, Q5)
    finally:
        brotli_amd.force_woff2_group_bytes(0)
    from_sizes = []
    room = 0
    for f in fonts:   # the groups the 400 KiB budget makes of the fonts that parse (woff2_batch.h's rule)
        if len(f) < 12 or f is rejected:
            continue
        if not from_sizes or len(f) > room:
            from_sizes.append(0)
            room = 400 * 1024
        from_sizes[-1] += 1
        room = max(0, room - len(f))
    assert len(from_sizes) >= 3
    for budget, out in results.items():
        assert len(out) == len(fonts)
        for i, (s, b) in enumerate(zip(solo, out)):
            if not isinstance(s, bytes):
                assert isinstance(b, brotli_amd.BrotliError) and b.code == s, (budget, i)
                continue
            assert isinstance(b, bytes), (budget, i, b)
            assert wf.parse(b)[:2] == wf.parse(s)[:2] and b[12:20] == s[12:20] and b[24:48] == s[24:48], (budget, i)
            assert _stream(b) == _stream(s), (budget, i)
            assert _decode(b) == _decode(s) and isinstance(_decode(b), bytes), (budget, i)


def test_empty_and_all_rejected_batches():
    """(that neither needs a device: tests/test_abi_woff2_encode.py, which runs without one)"""
    assert brotli_amd.woff2_encode_batch([]) == []
    out = brotli_amd.woff2_encode_batch([f for _, f in ww.rejected_fonts()])
    assert all(isinstance(e, brotli_amd.BrotliError) and e.code == wf.MIB_E_INVALID_ARG for e in out)


def test_profile_names(ttf):
    try:
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_encode_batch([ttf, ww.pack_cases()[0][1]], Q5)
        times = brotli_amd.default_kernel_times()
    finally:
        brotli_amd.default_profiling(False)
    assert times['w2enc_pack'][1] == 1   # one launch for both fonts
    for name in ('w2enc_glyf_sizes', 'w2enc_glyf_scan', 'w2enc_glyf_write', 'w2enc_hmtx_check', 'w2enc_hmtx_write'):
        assert times[name][1] == 1, name
    # the transform entry points alone report nothing of the kind
    try:
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_transform_glyf(ttf)
        assert not [k for k in brotli_amd.default_kernel_times() if k.startswith('w2enc')]
    finally:
        brotli_amd.default_profiling(False)


def test_node_woff2_encode():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_encode_test.js')], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
