"""woff2_decode / woff2_decode_batch of font collections on the GPU (flavor ttcf ->  a TTC;
brotli-lib_amd/csrc/woff2_file.hip, DESIGN.md 4c "A font collection"): the golden collections
decode to their golden TTCs byte for byte, alone and in batches beside single fonts; the
collections of the rejection list's items 14 - 20 give MIB_E_INVALID_ARG and no data; and the
assembly kernels alone (debug_ttc_assemble) agree with the Python assembler
(tests/_woff2_collection.assemble_collection) on the shapes at which a TTC can go wrong and a
single font cannot."""
import hashlib
import os
import shutil
import struct
import subprocess

import pytest

import _woff2_collection as wc
import _woff2_file as wf
import brotli_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = wc.golden_files()
SINGLE = {fx[0]: fx for fx in wf.golden_files()}
CASES = wc.kernel_cases()


def _solo(file):
    """what woff2_decode alone gives: the bytes, or the error's code"""
    try:
        return brotli_amd.woff2_decode(file)
    except brotli_amd.BrotliError as e:
        return e.code


def _plain(results):
    return [r.code if isinstance(r, brotli_amd.BrotliError) else r for r in results]


@pytest.mark.parametrize('name', [g[0] for g in GOLD])
def test_golden_decodes_to_its_ttc(name):
    """(without collections in the decoder this is MIB_E_INVALID_ARG)"""
    woff2, ttc = wc.golden_file(name)
    assert _solo(woff2) == ttc
    assert _plain(brotli_amd.woff2_decode_batch([woff2])) == [ttc]


def test_goldens_in_one_call():
    order = [2, 0, 1, 1, 0, 2, 2]
    out = _plain(brotli_amd.woff2_decode_batch([GOLD[g][1] for g in order]))
    assert out == [GOLD[g][2] for g in order]


def test_rejected_collections_alone_and_in_a_batch():
    cases = wc.rejected_collections()
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(14, 21))
    for name, file, _ in cases:
        assert _solo(file) == wf.MIB_E_INVALID_ARG, name
    files, good = [], []
    for i, (name, file, _) in enumerate(cases):
        files += [file, GOLD[i % 3][1]]
        good.append(GOLD[i % 3][2])
    out = _plain(brotli_amd.woff2_decode_batch(files))
    assert out[0::2] == [wf.MIB_E_INVALID_ARG] * len(cases)
    assert out[1::2] == good
    assert _plain(brotli_amd.woff2_decode_batch([c[1] for c in cases])) == [wf.MIB_E_INVALID_ARG] * len(cases)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_kernels_alone_agree_with_the_python_assembler(case):
    _, version, tables, fonts, misalign = case
    assert brotli_amd.debug_ttc_assemble(version, tables, fonts, misalign) == wc.assemble_collection(version, tables, fonts)


def test_kernel_cases_cover_the_shapes():
    ids = [c[0] for c in CASES]
    for want in ('1-fonts', '2-fonts', '3-fonts', '65-fonts', 'version-2', 'member-of-1-tables', 'member-of-64-tables',
                 'member-of-65-tables', 'shared-tables', 'shared-head', 'head-in-one-font', 'head-11-bytes',
                 'empty-shared-table', 'entry-no-font-lists', 'listed-in-another-order', 'sums-wrap') + \
            tuple('shared-tiles-plus-one-misalign-%d' % m for m in (0, 7, 15)):
        assert want in ids
    _, _, tables, fonts, _ = next(c for c in CASES if c[0] == 'shared-tables')
    ttc = wc.assemble_collection(wc.V1, tables, fonts)
    recs = [{r[0]: r for r in f[1]} for f in wc.read_ttc(ttc)[1]]
    assert recs[0][b'gvar'] == recs[1][b'gvar'] and recs[0][b'name'] != recs[1][b'name']


def test_shared_head_takes_the_last_fonts_value_on_every_run():
    _, version, tables, fonts, misalign = next(c for c in CASES if c[0] == 'shared-head-three-fonts')
    want = wc.assemble_collection(version, tables, fonts)
    # the expectation holds the last font's value, and the other fonts' values are others
    head = [i for i, (tag, _) in enumerate(tables) if tag == b'head'][0]
    assert all(head in idx for _, idx in fonts)
    values = []
    for (_, recs), start in zip(wc.read_ttc(want)[1], struct.unpack('>3L', want[12:24])):
        total = wf.checksum(want[start:start + 12 + 16 * len(recs)]) + sum(r[1] for r in recs)
        values.append((wf.HEAD_MAGIC - total) & 0xFFFFFFFF)
        at = next(r[2] for r in recs if r[0] == b'head')
    assert struct.unpack('>L', want[at + 8:at + 12])[0] == values[2] and values[2] not in values[:2]
    for _ in range(20):
        assert brotli_amd.debug_ttc_assemble(version, tables, fonts, misalign) == want


def test_debug_ttc_assemble_rejects_what_is_no_collection():
    tables = [(b'cmap', b'abc'), (b'name', b'defg'), (b'name', b'h')]
    for version, fonts in ((0x00030000, [(wc.V1, [0])]), (wc.V1, []), (wc.V1, [(wc.V1, [])]), (wc.V1, [(wc.V1, [3])]),
                           (wc.V1, [(wc.V1, [1, 2])]), (wc.V1, [(wc.V1, [0, 0])])):
        with pytest.raises(brotli_amd.BrotliError) as e:
            brotli_amd.debug_ttc_assemble(version, tables, fonts)
        assert e.value.code == wf.MIB_E_INVALID_ARG


def _groups(lens, budget):
    """woff2_batch.h make_groups, restated"""
    g, total, alone = [], 0, False
    for n in lens:
        big = n > budget
        if not g or alone or big or n > budget - total:
            g.append(0)
            total = 0
        g[-1] += 1
        total += 0 if big else n
        alone = big
    return g


def test_mixed_batch_at_the_default_grouping_and_in_three_groups():
    bad = next(c[1] for c in wc.rejected_collections() if c[0] == '16-index-at-numtables')
    single = SINGLE['synthetic-hmtx']
    files = [single[1], GOLD[1][1], bad, GOLD[2][1], single[1]]
    assert (GOLD[1][0], GOLD[2][0]) == ('ttc-shared-glyf', 'ttc-two-glyf')
    want = [single[2], GOLD[1][2], wf.MIB_E_INVALID_ARG, GOLD[2][2], single[2]]
    assert [_solo(f) for f in files] == want
    assert _plain(brotli_amd.woff2_decode_batch(files)) == want
    lens = [sum(wf.stream_lengths(wf.parse(single[1])[1]))]
    lens += [sum(wf.stream_lengths(wc.parse_collection(f)[1])) for f in (files[1], files[3])] + lens
    budget = next(b for b in sorted({a + c for a in lens for c in [0] + lens}) if len(_groups(lens, b)) == 3)
    brotli_amd.force_woff2_group_bytes(budget)
    try:
        assert _plain(brotli_amd.woff2_decode_batch(files)) == want
    finally:
        brotli_amd.force_woff2_group_bytes(0)


def test_bench_sized_collection_through_the_pair_loop():
    """two members share the glyf pair (and all else but one table) of the bench golden
    enc-ttf-hmtx.woff2: a real-sized glyf through the pair loop, the stream as the file has it"""
    name, file, _, size, sha = SINGLE['enc-ttf-hmtx']
    sfnt = brotli_amd.woff2_decode(file)
    assert len(sfnt) == size and hashlib.sha256(sfnt).hexdigest() == sha
    flavor, ent, comp = wf.parse(file)
    # (a collection wants loca right behind glyf; the transformed loca has no bytes in the
    # stream, so the entry moves and the stream stays)
    loca = next(e for e in ent if e[0] == b'loca')
    assert loca[3] == 0
    ent = [e for e in ent if e[0] != b'loca']
    ent.insert([e[0] for e in ent].index(b'glyf') + 1, loca)
    tags = [e[0] for e in ent]
    assert ent[tags.index(b'hmtx')][1] == 1 and ent[tags.index(b'glyf')][3] > 100 * 1024   # (the bench font's: 118,851)
    tables = wf.sfnt_tables(sfnt)
    fonts = [(flavor, list(range(len(ent)))), (wc.TRUE, [i for i in reversed(range(len(ent))) if tags[i] != b'name'])]
    woff2 = wc.write_collection(wc.V2, ent, fonts, comp)
    want = wc.assemble_collection(wc.V2, [(tag, tables[tag]) for tag in tags], fonts)
    assert _solo(woff2) == want
    assert _plain(brotli_amd.woff2_decode_batch([file, woff2])) == [sfnt, want]


def test_a_flipped_stream_byte_never_returns_data():
    """(the two collections whose streams are compressed data at the flipped byte: in ttc-null's
    the byte is a literal, and the stream still decodes to its length)"""
    for name, woff2, _ in GOLD[1:]:
        comp = wc.parse_collection(woff2)[3]
        b = bytearray(woff2)
        b[len(woff2) - len(comp) + len(comp) // 2] ^= 0x5A
        out = _solo(bytes(b))
        assert isinstance(out, int) and out < 0, name
        assert _plain(brotli_amd.woff2_decode_batch([woff2, bytes(b)]))[1] == out, name


def test_node_woff2_collection():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_collection_test.js')], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
