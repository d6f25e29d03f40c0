"""woff2_decode_batch on the GPU (brotli-lib_amd/csrc/woff2_file.hip, woff2_batch.h): a call over
many .woff2 files gives per slot what woff2_decode of that file alone gives -- the golden sfnts,
the codes of the rejection list next to good files, files written around the product's own
transforms and encoder, more files than the GPU has compute units, the same results however the
call is cut into groups -- with one launch of the decode, the peek, the hmtx and each assembly
kernel per group; and the batched assembly kernels alone agree with the Python assembler
(tests/_woff2_file.assemble) on the shapes at which a launch over several fonts can go wrong and
a launch over one cannot."""
import hashlib
import json
import os
import random
import shutil
import struct
import subprocess

import pytest

import _oracle
import _woff2_file as wf
import brotli_amd
from brotli_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = wf.golden_files()
SYN = {fx[0]: fx for fx in GOLD[:2]}


def _font_q11(data):
    return brotli_amd.brotliEncode(data, {'quality': 11, 'mode': brotli_amd.EncoderMode.FONT})


def _is_golden(out, fx):
    name, _, sfnt, size, sha = fx
    assert isinstance(out, bytes), (name, out)
    assert len(out) == size and hashlib.sha256(out).hexdigest() == sha, name
    if sfnt is not None:
        assert out == sfnt, name


def _solo(file):
    """what woff2_decode alone gives: the bytes, or the error's code"""
    try:
        return brotli_amd.woff2_decode(file)
    except brotli_amd.BrotliError as e:
        return e.code


def _stream_len(file):
    return sum(wf.stream_lengths(wf.parse(file)[1]))


def test_fixture_names():
    assert sorted(SYN) == ['synthetic', 'synthetic-hmtx'] and len(GOLD) == 7


def test_goldens_in_one_call():
    order = list(range(len(GOLD))) + [4]
    random.Random(3).shuffle(order)
    out = brotli_amd.woff2_decode_batch([GOLD[g][1] for g in order])
    assert len(out) == len(order)
    for g, o in zip(order, out):
        _is_golden(o, GOLD[g])
    solo = {name: brotli_amd.woff2_decode(fx[1]) for name, fx in SYN.items()}
    for g, o in zip(order, out):
        if GOLD[g][0] in solo:
            assert o == solo[GOLD[g][0]]
    assert brotli_amd.woff2_decode_batch([SYN['synthetic-hmtx'][1]]) == [solo['synthetic-hmtx']]


def _bad_files():
    """[(id, file)]: the first case of every item of the rejection list, an empty file, and a file
    with a byte of its Brotli stream flipped"""
    seen, out = set(), []
    for name, file, stream, edited in wf.rejected_files(_oracle.decode):
        item = int(name.split('-')[0])
        if item in seen:
            continue
        seen.add(item)
        out.append((name, wf.with_stream(file, stream, _font_q11) if edited else file))
    assert sorted(seen) == list(range(1, 14))
    out.append(('empty', b''))
    good = SYN['synthetic-hmtx'][1]
    _, ent, comp = wf.parse(good)
    start = len(wf.write(0, ent, b''))
    assert good[start:start + len(comp)] == comp
    b = bytearray(good)
    b[start + len(comp) // 2] ^= 0x5A
    out.append(('flipped-byte', bytes(b)))
    return out


def test_bad_files_keep_their_codes_and_leave_the_good_ones_alone():
    """woff2_decode is the batch with one file, so the codes are pinned: decode_codes.json holds
    what woff2_decode gave for each of these files while it still was a path of its own"""
    bad = _bad_files()
    with open(os.path.join(wf.HERE, 'decode_codes.json')) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(name for name, _ in bad)
    assert all(code == wf.MIB_E_INVALID_ARG for name, code in recorded.items() if name != 'flipped-byte')
    files, kind = [], []
    for i, (name, file) in enumerate(bad):
        files.append(file)
        kind.append(None)
        files.append(GOLD[i % 2][1])
        kind.append(i % 2)
    out = brotli_amd.woff2_decode_batch(files)
    assert len(out) == len(files)
    for (name, file), o in zip(bad, out[0::2]):
        want = recorded[name]
        assert isinstance(want, int) and want < 0, name
        assert _solo(file) == want, name
        assert isinstance(o, brotli_amd.BrotliError) and o.code == want, (name, o, want)
    for g, o in zip(kind[1::2], out[1::2]):
        _is_golden(o, GOLD[g])
    assert brotli_amd.woff2_decode(GOLD[1][1]) == GOLD[1][2]


def test_files_made_by_the_product():
    """the engine's own FONT-mode q11 streams: a small glyph count, one that is no multiple of the
    reconstruct kernels' 256 threads, and one that is"""
    files, wants, fonts = [], [], []
    for seed, glyphs in ((11, 5), (12, 300), (13, 512)):
        ttf = wf.font_with_metrics(datagen.glyf_font(seed, glyphs))
        file, want = wf.product_file(ttf, brotli_amd.woff2_transform_glyf, brotli_amd.woff2_transform_hmtx,
                                     brotli_amd.woff2_reconstruct_glyf, _font_q11)
        files.append(file), wants.append(want), fonts.append(ttf)
    out = brotli_amd.woff2_decode_batch(files)
    for o, want, ttf in zip(out, wants, fonts):
        assert o == want
        assert wf.sfnt_tables(o)[b'hmtx'] == wf.sfnt_tables(ttf)[b'hmtx']


def test_more_files_than_compute_units():
    k = 257
    assert sum(_stream_len(GOLD[i % 2][1]) for i in range(k)) < 512 << 20   # one group
    out = brotli_amd.woff2_decode_batch([GOLD[i % 2][1] for i in range(k)])
    assert len(out) == k
    for i, o in enumerate(out):
        assert o == GOLD[i % 2][2], i


def test_one_launch_of_each_shared_kernel_per_group():
    files = [SYN['synthetic-hmtx'][1], SYN['synthetic'][1], SYN['synthetic-hmtx'][1]]
    try:
        brotli_amd.default_profiling(True)
        one = brotli_amd.woff2_decode_batch(files[:1])
        times_one = brotli_amd.default_kernel_times()
        brotli_amd.default_profiling(True)
        out = brotli_amd.woff2_decode_batch(files)
        times = brotli_amd.default_kernel_times()
    finally:
        brotli_amd.default_profiling(False)
    assert one == [SYN['synthetic-hmtx'][2]]
    assert out == [SYN['synthetic-hmtx'][2], SYN['synthetic'][2], SYN['synthetic-hmtx'][2]]
    print(times)
    for name in ('w2file_assemble', 'w2file_directory', 'w2inv_hmtx', 'w2file_peek'):
        assert times[name][1] == 1, (name, times)
    decode = sorted(k for k in times if k.startswith('decode_'))
    assert decode and decode == sorted(k for k in times_one if k.startswith('decode_'))
    for name in decode:
        assert times[name][1] == times_one[name][1], (name, times, times_one)
    # the glyf reconstruct runs per font
    assert times['w2inv_write'][1] == 3 and times_one['w2inv_write'][1] == 1


def test_groups_give_the_one_group_results():
    big = next(fx for fx in GOLD if fx[0] == 'enc-otf')
    a, b = SYN['synthetic'], SYN['synthetic-hmtx']
    files = [a[1], b[1], big[1], b[1], a[1]]
    lens = [_stream_len(f) for f in files]
    budget = lens[0] + lens[1]
    assert lens[2] > budget   # [a b] [big, alone above the budget] [b a]: three groups
    whole = brotli_amd.woff2_decode_batch(files)
    for o, fx in zip(whole, (a, b, big, b, a)):
        _is_golden(o, fx)
    try:
        brotli_amd.force_woff2_group_bytes(budget)
        assert brotli_amd.woff2_decode_batch(files) == whole
        brotli_amd.force_woff2_group_bytes(1)   # every file a group alone
        assert brotli_amd.woff2_decode_batch(files) == whole
    finally:
        brotli_amd.force_woff2_group_bytes(0)
    assert brotli_amd.woff2_decode_batch(files) == whole


# ---------------------------------------------------------------- the assembly kernels alone
def _tables(k, salt, lens=None):
    return [(b'T%03d' % (k - i), wf._blob(lens[i] if lens else 3 * i + 1, salt + i)) for i in range(k)]


def _many_small_tables():
    fonts = []
    for f in range(8):
        fonts.append((0x00010000, [(struct.pack('>L', 0x41000000 + i), wf._blob(1 + (i + f) % 3, i + 7 * f)) for i in range(8250)]))
    return fonts


def assemble_batch_cases():
    """[(id, [(flavor, [(tag, bytes)])], misalign or None)]"""
    head = wf._head(54, 9)
    others = [(b'cmap', wf._blob(40, 1)), (b'maxp', wf._blob(32, 2)), (b'post', wf._blob(21, 3))]
    ttf, otf = 0x00010000, 0x4F54544F
    c = []
    c.append(('table-counts-1-2-17-65-130', [(ttf, _tables(k, k)) for k in (1, 2, 17, 65, 130)], None))
    c.append(('130-tables-first', [(otf, _tables(k, k)) for k in (130, 1, 65)], None))
    c.append(('same-tags-other-bytes', [(ttf, _tables(5, 1)), (ttf, _tables(5, 100))], None))
    c.append(('head-in-the-first-font-only', [(ttf, [(b'head', head)] + others), (ttf, others), (otf, others[:2])], None))
    c.append(('head-in-the-last-font-only', [(ttf, others), (otf, others[:2]), (ttf, others + [(b'head', head)])], None))
    c.append(('head-11-and-12-bytes', [(ttf, [(b'cmap', wf._blob(5, 4)), (b'head', wf._head(11, 5))]),
                                       (ttf, [(b'head', wf._head(12, 5)), (b'cmap', wf._blob(5, 4))]),
                                       (ttf, [(b'head', wf._head(11, 6))]), (ttf, [(b'head', wf._head(12, 7))])], None))
    c.append(('empty-last-table-then-a-font', [(ttf, [(b'cmap', wf._blob(9, 1)), (b'post', b'')]), (ttf, [(b'cmap', wf._blob(7, 2))]),
                                               (ttf, [(b'post', b'')]), (otf, others)], None))
    c.append(('first-table-misaligned-0-15', [(ttf, [(b'name', wf._blob(33, m)), (b'post', wf._blob(33, m + 16))]) for m in range(16)],
              [[m, (m + 5) & 15] for m in range(16)]))
    c.append(('sfnt-length-12-mod-16', [(ttf, [(b'cmap', wf._blob(16, 1))]), (ttf, [(b'cmap', wf._blob(16, 2))]), (ttf, others)], None))
    c.append(('tile-spread', [(ttf, [(b'cmap', b'\x01')]), (ttf, [(b'aaaa', b'\x02'), (b'gvar', wf._blob(70 * 4096 + 18, 5)), (b'zzzz', b'\x03')]),
                              (ttf, [(b'post', b'\x04'), (b'head', wf._head(54, 6))])], [[3], [1, 7, 2], None]))
    c.append(('more-than-65535-tables', _many_small_tables(), None))
    return c


ASSEMBLE = assemble_batch_cases()


def test_assemble_cases_are_what_they_say():
    by = {c[0]: c for c in ASSEMBLE}
    assert len(wf.assemble(*by['sfnt-length-12-mod-16'][1][0])) % 16 == 12
    assert sum(len(t) for _, t in by['more-than-65535-tables'][1]) > 65535
    assert [len(t) for _, t in by['table-counts-1-2-17-65-130'][1]] == [1, 2, 17, 65, 130]


@pytest.mark.parametrize('case', ASSEMBLE, ids=lambda c: c[0])
def test_batched_assembly_kernels_match_the_python_assembler(case):
    name, fonts, misalign = case
    out = brotli_amd.debug_sfnt_assemble_batch(fonts, misalign)
    assert len(out) == len(fonts)
    for f, ((flavor, tables), got) in enumerate(zip(fonts, out)):
        want = wf.assemble(flavor, tables)
        if got != want:
            d = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            pytest.fail('font %d: %d bytes, expected %d; first difference at %d: %s vs %s' %
                        (f, len(got), len(want), d, got[d:d + 16].hex(), want[d:d + 16].hex()))


def test_batched_assembly_is_the_same_on_every_run():
    """the table sums are accumulated with atomic adds, whose order is free: the sums wrap"""
    _, fonts, misalign = next(c for c in ASSEMBLE if c[0] == 'tile-spread')
    first = brotli_amd.debug_sfnt_assemble_batch(fonts, misalign)
    assert all(brotli_amd.debug_sfnt_assemble_batch(fonts, misalign) == first for _ in range(3))


def test_node_woff2_decode_batch():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_decode_batch_test.js')], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
