"""GPU inverse WOFF2 transforms (brotli-lib_amd/csrc/woff2_inv.hip): woff2_reconstruct_glyf is
byte-exact with fontTools on the fixtures of tests/golden/woff2/reconstruct_golden.json and on
the bench fonts; the forward transform of what it reconstructs is the table it started from
(no fontTools needed); woff2_reconstruct_hmtx gives the fonts' hmtx tables back; tables that
do not parse raise MIB_E_INVALID_ARG."""
import hashlib
import os
import shutil
import struct
import subprocess
import sys

import pytest

import _oracle  # noqa: F401
import _woff2_reconstruct as w2
import brotli_amd
from brotli_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, w2.HERE)
MIB_E_INVALID_ARG = -101


def sfnt(tglyf, glyf, loca):
    """A four-table TrueType font (head, maxp, glyf, loca: all woff2_transform_glyf reads) around
    reconstructed tables; indexToLocFormat and numGlyphs from the transformed table's header."""
    ng, fmt = struct.unpack('>HH', tglyf[4:8])
    head = bytearray(54)
    head[50:52] = struct.pack('>h', fmt)
    maxp = struct.pack('>LH', 0x00010000, ng)
    tables = sorted({b'head': bytes(head), b'maxp': maxp, b'glyf': glyf, b'loca': loca}.items())
    out = bytearray(struct.pack('>LHHHH', 0x00010000, len(tables), 64, 2, 0))
    pos = 12 + 16 * len(tables)
    body = b''
    for tag, data in tables:
        out += tag + struct.pack('>LLL', 0, pos + len(body), len(data))
        body += data + b'\0' * (-len(data) % 4)
    return bytes(out) + body


@pytest.fixture(scope='module')
def inputs():
    """{name: transformed glyf}: the synthetic fixtures, the bench fonts and two generated fonts
    (the latter through the forward kernels, which the fontTools goldens pin)"""
    import make_golden
    t = {name: fx['tglyf'] for name, fx in w2.synthetic().items()}
    for name, ttf in make_golden.fonts():
        t[name] = brotli_amd.woff2_transform_glyf(ttf)
    for seed in (41, 42):
        t['datagen-%d' % seed] = brotli_amd.woff2_transform_glyf(datagen.glyf_font(seed, 800))
    return t


@pytest.fixture(scope='module')
def rebuilt(inputs):
    return {name: brotli_amd.woff2_reconstruct_glyf(t) for name, t in inputs.items()}


def test_reconstructed_glyf_matches_fonttools(inputs, rebuilt):
    gold = w2.golden()['bench']
    for name, fx in w2.synthetic().items():
        glyf, loca = rebuilt[name]
        assert glyf == fx['glyf'], name
        assert loca == fx['loca'], name
    for name, g in gold.items():
        assert hashlib.sha256(inputs[name]).hexdigest() == g['tglyf_sha256'], name
        glyf, loca = rebuilt[name]
        assert (len(glyf), len(loca)) == (g['glyf_size'], g['loca_size']), name
        assert hashlib.sha256(glyf).hexdigest() == g['glyf_sha256'], name
        assert hashlib.sha256(loca).hexdigest() == g['loca_sha256'], name


def test_forward_transform_of_the_reconstruction_is_the_input(inputs, rebuilt):
    assert len(inputs) == 6
    for name, t in inputs.items():
        glyf, loca = rebuilt[name]
        assert brotli_amd.woff2_transform_glyf(sfnt(t, glyf, loca)) == t, name


def test_all_empty_font_is_one_zero_byte():
    """fontTools writes a single zero byte when every glyph is empty; loca is all zeros"""
    t, glyf, loca = w2.all_empty()
    assert brotli_amd.woff2_reconstruct_glyf(t) == (glyf, loca)


def test_reconstructed_hmtx_is_the_fonts_hmtx(rebuilt):
    import make_golden
    seen = 0
    for name, ttf in make_golden.fonts():
        for tag, v in make_golden.hmtx_variants(ttf):
            if tag == 'both':
                continue   # no transform applies: nothing to reconstruct
            ng = struct.unpack('>H', v[make_golden._table(v, b'maxp')[0] + 4:][:2])[0]
            nhm = struct.unpack('>H', v[make_golden._table(v, b'hhea')[0] + 34:][:2])[0]
            off, length = make_golden._table(v, b'hmtx')
            glyf, loca = brotli_amd.woff2_reconstruct_glyf(brotli_amd.woff2_transform_glyf(v))
            assert (glyf, loca) == rebuilt[name]
            th = brotli_amd.woff2_transform_hmtx(v)
            assert brotli_amd.woff2_reconstruct_hmtx(th, glyf, loca, ng, nhm) == v[off:off + length], (name, tag)
            seen += 1
    assert seen == 6
    for name, fx in w2.synthetic().items():
        glyf, loca = rebuilt[name]
        got = brotli_amd.woff2_reconstruct_hmtx(fx['thmtx'], glyf, loca, fx['num_glyphs'], fx['num_hmetrics'])
        assert got == fx['hmtx'], name


@pytest.mark.parametrize('case', w2.bad_inputs(), ids=lambda c: c[0])
def test_bad_tables_are_invalid_arg(case):
    """the error path reaches the caller (the CPU tests already saw the walker reject these)"""
    _, kind, table, fx = case
    with pytest.raises(brotli_amd.BrotliError) as e:
        if kind == 'glyf':
            brotli_amd.woff2_reconstruct_glyf(table)
        else:
            brotli_amd.woff2_reconstruct_hmtx(table, fx['glyf'], fx['loca'], fx['num_glyphs'], fx['num_hmetrics'])
    assert e.value.code == MIB_E_INVALID_ARG


def test_offsets_beyond_a_short_loca_are_invalid_arg(inputs, rebuilt):
    """enc-ttf's 140 KB of glyphs under indexFormat 0 (the CPU tests saw the walker reject it)"""
    assert len(rebuilt['enc-ttf'][0]) >= 0x20000
    with pytest.raises(brotli_amd.BrotliError) as e:
        brotli_amd.woff2_reconstruct_glyf(w2.with_short_loca(inputs['enc-ttf']))
    assert e.value.code == MIB_E_INVALID_ARG


def test_node_reconstruct():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_reconstruct_test.js')], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
