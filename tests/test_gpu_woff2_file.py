"""woff2_decode on the GPU (brotli-lib_amd/csrc/woff2_file.hip): every golden .woff2 file of
tests/golden/woff2/file_golden.json becomes its golden sfnt; the assembly kernels alone agree
with the Python assembler (tests/_woff2_file.assemble, which the CPU tests hold against
host_assemble) on the sizes, alignments and table counts at which they take another path; a file
written around the product's own transforms and encoder decodes to what the assembler expects;
every item of the rejection list is MIB_E_INVALID_ARG and leaves the default context usable;
the refactored reconstruct entry points still report the kernels they reported."""
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

import _oracle
import _woff2_file as wf
import brotli_amd
from brotli_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, wf.HERE)
W2INV_GLYF_KERNELS = ['w2inv_chain', 'w2inv_comp', 'w2inv_count', 'w2inv_loca', 'w2inv_measure', 'w2inv_npoints',
                      'w2inv_scan_counts', 'w2inv_scan_instr', 'w2inv_scan_points', 'w2inv_scan_sizes', 'w2inv_size',
                      'w2inv_write']


def _font_q11(data):
    return brotli_amd.brotliEncode(data, {'quality': 11, 'mode': brotli_amd.EncoderMode.FONT})


@pytest.fixture(scope='module')
def good():
    """(file, sfnt) that must still decode after every error"""
    name, data, sfnt, _, _ = wf.golden_files()[1]
    assert name == 'synthetic-hmtx'
    return data, sfnt


@pytest.mark.parametrize('fx', wf.golden_files(), ids=lambda fx: fx[0])
def test_golden_file_decodes_to_its_sfnt(fx):
    name, data, sfnt, size, sha = fx
    out = brotli_amd.woff2_decode(data)
    assert len(out) == size
    assert hashlib.sha256(out).hexdigest() == sha
    if sfnt is not None:
        assert out == sfnt


@pytest.mark.parametrize('case', wf.assemble_cases(), ids=lambda c: c[0])
def test_assembly_kernels_match_the_python_assembler(case):
    _, flavor, tables, misalign = case
    out = brotli_amd.debug_sfnt_assemble(flavor, tables, misalign)
    want = wf.assemble(flavor, tables)
    if out != want:
        d = next((i for i in range(min(len(out), len(want))) if out[i] != want[i]), min(len(out), len(want)))
        pytest.fail('%d bytes, expected %d; first difference at %d: %s vs %s' %
                    (len(out), len(want), d, out[d:d + 16].hex(), want[d:d + 16].hex()))


def test_assembly_is_the_same_on_every_run():
    """the table sums are accumulated with atomic adds, whose order is free: the sums wrap"""
    _, flavor, tables, misalign = next(c for c in wf.assemble_cases() if c[0] == 'tiles-many')
    first = brotli_amd.debug_sfnt_assemble(flavor, tables, misalign)
    assert all(brotli_amd.debug_sfnt_assemble(flavor, tables, misalign) == first for _ in range(3))


def test_file_made_by_the_product_decodes():
    """the engine's own FONT-mode q11 stream next to the oracle-made ones of the goldens"""
    ttf = wf.font_with_metrics(datagen.glyf_font(41, 800))
    file, want = wf.product_file(ttf, brotli_amd.woff2_transform_glyf, brotli_amd.woff2_transform_hmtx,
                                 brotli_amd.woff2_reconstruct_glyf, _font_q11)
    out = brotli_amd.woff2_decode(file)
    assert out == want
    # hmtx went through its transform and came back as the font's own
    assert wf.sfnt_tables(out)[b'hmtx'] == wf.sfnt_tables(ttf)[b'hmtx']


REJECTED = wf.rejected_files(_oracle.decode)


@pytest.mark.parametrize('case', REJECTED, ids=lambda c: c[0])
def test_rejected_file_is_invalid_arg(case, good):
    _, file, stream, edited = case
    if edited:   # a container that parses around a table that does not
        file = wf.with_stream(file, stream, _font_q11)
    with pytest.raises(brotli_amd.BrotliError) as e:
        brotli_amd.woff2_decode(file)
    assert e.value.code == wf.MIB_E_INVALID_ARG
    assert brotli_amd.woff2_decode(good[0]) == good[1]


def test_rejection_list_is_complete():
    assert sorted({int(c[0].split('-')[0]) for c in REJECTED}) == list(range(1, 14))


def test_flipped_byte_in_the_brotli_stream_never_returns_data(good):
    file = good[0]
    _, ent, comp = wf.parse(file)
    start = len(wf.write(0, ent, b''))
    assert file[start:start + len(comp)] == comp
    seen = set()
    for at in (0, 1, len(comp) // 3, len(comp) // 2, len(comp) - 2):
        b = bytearray(file)
        b[start + at] ^= 0x5A
        with pytest.raises(brotli_amd.BrotliError) as e:
            brotli_amd.woff2_decode(bytes(b))
        assert e.value.code == wf.MIB_E_INVALID_ARG or -30 <= e.value.code <= -1, e.value.code
        seen.add(e.value.code)
        assert brotli_amd.woff2_decode(file) == good[1]
    print('codes', sorted(seen))


def test_profile_names_of_the_new_and_the_old_entry_points():
    import make_golden
    name, ttf = next(iter(make_golden.fonts()))
    assert name == 'enc-ttf'
    tglyf = brotli_amd.woff2_transform_glyf(ttf)
    thmtx = brotli_amd.woff2_transform_hmtx(ttf)
    glyf, loca = brotli_amd.woff2_reconstruct_glyf(tglyf)
    ng = int.from_bytes(tglyf[4:6], 'big')
    nhm = int.from_bytes(wf.sfnt_tables(ttf)[b'hhea'][34:36], 'big')
    data = next(fx[1] for fx in wf.golden_files() if fx[0] == 'enc-ttf-hmtx')
    try:
        # the transform wrappers run with the timer off: they report nothing
        brotli_amd.default_profiling(True)
        assert brotli_amd.woff2_transform_glyf(ttf) == tglyf
        assert sorted(brotli_amd.default_kernel_times()) == []
        brotli_amd.default_profiling(True)
        assert brotli_amd.woff2_transform_hmtx(ttf) == thmtx
        assert sorted(brotli_amd.default_kernel_times()) == []
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_reconstruct_glyf(tglyf)
        assert sorted(brotli_amd.default_kernel_times()) == W2INV_GLYF_KERNELS
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_reconstruct_hmtx(thmtx, glyf, loca, ng, nhm)
        assert {k: v[1] for k, v in brotli_amd.default_kernel_times().items()} == {'w2inv_hmtx': 1}
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_decode(data)
        times = brotli_amd.default_kernel_times()
        assert times['w2file_assemble'][1] == 1 and times['w2file_directory'][1] == 1
        assert times['w2file_peek'][1] == 1   # woff2_decode is the batch with one file
        assert any(k.startswith('decode_') for k in times)   # the Brotli stream, on the same context
        assert sorted(k for k in times if k.startswith('w2inv_')) == sorted(W2INV_GLYF_KERNELS + ['w2inv_hmtx'])
    finally:
        brotli_amd.default_profiling(False)


def test_node_woff2_decode():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_decode_test.js')], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
