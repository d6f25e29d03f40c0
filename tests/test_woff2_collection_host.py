"""WOFF2 font collections (flavor ttcf) without a GPU: the CollectionHeader parser, the
collection plan and the serial assembly of brotli-lib_amd/csrc/woff2_file.h / woff2_batch.h, built
as host code with AddressSanitizer and UBSan into a stand-alone program
(tests/woff2_collection_host_main.cpp), turn every golden collection and its oracle-decoded
stream into the golden TTC, reject every case of items 14 - 21 of the rejection list, run single
fonts and collections mixed through the batch plan, take damaged collections without a report or
a broken plan, and agree with the Python assembler that the GPU test measures the kernels
against.  fontTools, which cannot read WOFF2 collections but reads TTCs, opens every member of
every golden TTC with its checksums verified."""
import hashlib
import io
import os
import shutil
import struct
import subprocess
import sys

import pytest

import _oracle
import _woff2_collection as wc
import _woff2_file as wf
import _woff2_reconstruct as w2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, wf.HERE)

FUZZ_SEED = 20240611
FUZZ_DOUBLES = 4000   # random double edits per golden file, beside the structured damage
NAMES = ['ttc-null', 'ttc-shared-glyf', 'ttc-two-glyf']


def test_goldens_are_the_generators_output():
    """the generator gives the committed JSON again"""
    pytest.importorskip('fontTools')
    import make_collection_golden
    assert make_collection_golden.generate() == wc.golden()


def test_fixtures_are_what_they_are_named_and_stay_small():
    g = wc.golden()['files']
    assert sorted(g) == NAMES
    assert os.path.getsize(os.path.join(wf.HERE, 'collection_golden.json')) < 256 * 1024
    for name, fx in g.items():
        assert fx['code'] == 0
        woff2, ttc = wc.golden_file(name)
        assert len(woff2) == fx['woff2_size'] and hashlib.sha256(woff2).hexdigest() == fx['woff2_sha256']
        assert len(ttc) == fx['ttc_size'] and hashlib.sha256(ttc).hexdigest() == fx['ttc_sha256']
    state = lambda e: wf.is_transformed(e[0], e[1])   # noqa: E731
    v, ent, fonts, _ = wc.parse_collection(wc.golden_file('ttc-shared-glyf')[0])
    assert v == wc.V1 and len(fonts) == 2
    both = set(fonts[0][1]) & set(fonts[1][1])
    assert {ent[i][0] for i in both if state(ent[i])} == {b'glyf', b'loca', b'hmtx'} and b'hhea' in {ent[i][0] for i in both}
    assert [[ent[i][0] for i in idx if i not in both] for _, idx in fonts] == [[b'name'], [b'name']]
    v, ent, fonts, _ = wc.parse_collection(wc.golden_file('ttc-two-glyf')[0])
    assert v == wc.V2 and len(fonts) == 2 and fonts[0][0] != fonts[1][0] and not set(fonts[0][1]) & set(fonts[1][1])
    for _, idx in fonts:
        assert {ent[i][0] for i in idx if state(ent[i])} >= {b'glyf', b'loca'}
    assert sorted(b'hmtx' in {ent[i][0] for i in idx if state(ent[i])} for _, idx in fonts) == [False, True]
    assert len(set(range(len(ent))) - set(fonts[0][1]) - set(fonts[1][1])) == 1
    v, ent, fonts, _ = wc.parse_collection(wc.golden_file('ttc-null')[0])
    assert len(fonts) == 1 and {e[0]: e[1] for e in ent}[b'glyf'] == 3 and {e[0]: e[1] for e in ent}[b'loca'] == 3
    assert b'head' in {ent[i][0] for i in fonts[0][1]}


def test_container_writer_and_parser_agree():
    for name, woff2, _ in wc.golden_files():
        assert wc.write_collection(*wc.parse_collection(woff2)) == woff2, name
    for v in list(range(0, 1000)) + [65535]:
        assert wc._read255(wc.u255(v) + b'\0\0', 0) == (v, len(wc.u255(v)))
        assert wc._read255(wc.u255_word(v), 0) == (v, 3)


def test_single_font_with_its_flavor_patched_is_still_rejected(driver, tmp_path):
    """the existing case 1-flavor-ttcf: whatever the CollectionHeader parse takes from the
    Brotli stream's first bytes, totalCompressedSize then runs past the file"""
    cases = [c for c in wf.rejected_files(_oracle.decode) if c[0] == '1-flavor-ttcf']
    assert len(cases) == 1
    for hm in (False, True):
        b = bytearray(wf.synthetic_file(hm))
        b[4:8] = b'ttcf'
        cases.append(('patched', bytes(b), _oracle.decode(wf.parse(wf.synthetic_file(hm))[2]), False))
    for rc, out in _assemble(driver, tmp_path, [(file, stream) for _, file, stream, _ in cases]):
        assert rc == -1 and out == b''


def test_fonttools_opens_every_member():
    """checkChecksums=2 asserts every record's checksum (and the font's sum with its head)"""
    pytest.importorskip('fontTools')
    from fontTools.ttLib.sfnt import SFNTReader
    for name, woff2, ttc in wc.golden_files():
        _, ent, fonts, comp = wc.parse_collection(woff2)
        for m, (flavor, idx) in enumerate(fonts):
            r = SFNTReader(io.BytesIO(ttc), checkChecksums=2, fontNumber=m)
            assert sorted(r.keys()) == sorted(ent[i][0].decode('latin-1') for i in idx), (name, m)
            mine = wc.member_tables(ttc, m)
            for tag in r.keys():
                assert r[tag] == mine[tag.encode('latin-1')], (name, m, tag)


def test_members_equal_their_single_font_expectation():
    """each member's tables are, tag by tag, those of the sfnt that the same font alone stands
    for: the member written as a single-font .woff2 from the collection's own directory entries
    and stream bytes, its expectation assembled from the same reconstructed tables"""
    for name, woff2, ttc in wc.golden_files():
        version, ent, fonts, comp = wc.parse_collection(woff2)
        assert wc.read_ttc(ttc)[0] == version
        assert [fl for fl, _ in wc.read_ttc(ttc)[1]] == [fl for fl, _ in fonts]
        for m, (flavor, idx) in enumerate(fonts):
            mine = wc.member_tables(ttc, m)
            assert sorted(mine) == sorted(ent[i][0] for i in idx)
            single = wf.assemble(flavor, [(ent[i][0], mine[ent[i][0]]) for i in sorted(idx)])
            theirs = wf.sfnt_tables(single)
            for tag in mine:
                if tag == b'head':   # (checkSumAdjustment is the file's: all else equal)
                    assert mine[tag][:8] + mine[tag][12:] == theirs[tag][:8] + theirs[tag][12:], (name, m)
                else:
                    assert mine[tag] == theirs[tag], (name, m, tag)


def test_members_equal_the_reconstructed_single_font(driver, tmp_path):
    """... and of the sfnt the host assembly gives for the member as a single-font file"""
    pairs, keys = [], []
    for name, woff2, ttc in wc.golden_files():
        version, ent, fonts, comp = wc.parse_collection(woff2)
        parts = wc.cut_list(ent, _oracle.decode(comp))
        for m, (flavor, idx) in enumerate(fonts):
            order = sorted(idx)
            pairs.append((wf.write(flavor, [ent[i] for i in order], b''), b''.join(parts[i] for i in order)))
            keys.append((name, m, ttc))
    got = _assemble(driver, tmp_path, pairs)
    for (name, m, ttc), (rc, sfnt) in zip(keys, got):
        assert rc == 0, (name, m)
        mine, theirs = wc.member_tables(ttc, m), wf.sfnt_tables(sfnt)
        assert sorted(mine) == sorted(theirs)
        for tag in mine:
            if tag == b'head':
                assert mine[tag][:8] + mine[tag][12:] == theirs[tag][:8] + theirs[tag][12:], (name, m)
            else:
                assert mine[tag] == theirs[tag], (name, m, tag)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_collection') / 'woff2_collection_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_collection_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _records(tmp_path, pairs):
    src = str(tmp_path / 'in.bin')
    with open(src, 'wb') as f:
        for file, stream in pairs:
            f.write(w2.record(file) + w2.record(stream))
    return src


def _assemble(exe, tmp_path, pairs):
    """[(return code, TTC or sfnt)] of host_assemble over [(file, stream)]"""
    src, dst = _records(tmp_path, pairs), str(tmp_path / 'out.bin')
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
    return _oracle.decode(wc.parse_collection(file)[3])


def test_host_assembly_matches_the_goldens(driver, tmp_path):
    gold = wc.golden_files()
    got = _assemble(driver, tmp_path, [(woff2, _stream_of(woff2)) for _, woff2, _ in gold])
    for (name, _, ttc), (rc, out) in zip(gold, got):
        assert rc == 0, name
        assert out == ttc, name


def test_host_parser_rejects_the_list(driver, tmp_path):
    cases = wc.rejected_collections()
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(14, 21))
    streams = {name: _stream_of(woff2) for name, woff2, _ in wc.golden_files()}
    got = _assemble(driver, tmp_path, [(file, streams[base]) for _, file, base in cases])
    for (name, _, _), (rc, out) in zip(cases, got):
        assert rc == -1 and out == b'', name
    assert _run(driver, 'layout').strip() == 'layout ok'   # item 21


def test_the_list_is_rejected_for_its_own_reasons(driver, tmp_path):
    """the edits' counterparts that stay inside the rules are accepted: an index of numTables - 1
    in every 255UInt16 form, the members in another order, a member listed twice"""
    woff2, ttc = wc.golden_file('ttc-shared-glyf')
    v, ent, fonts, comp = wc.parse_collection(woff2)
    stream = _oracle.decode(comp)
    parts = wc.cut_list(ent, stream)
    want = {i: wc.member_tables(ttc, m)[ent[i][0]] for m, (_, idx) in enumerate(fonts) for i in idx}
    tables = [(ent[i][0], want[i]) for i in range(len(ent))]
    assert wc.assemble_collection(v, tables, fonts) == ttc
    variants = [
        [(fl, [wc.u255_word(i) for i in idx]) for fl, idx in fonts],
        list(reversed(fonts)),
        fonts + [fonts[0]],
        [(fl, list(reversed(idx))) for fl, idx in fonts],
    ]
    got = _assemble(driver, tmp_path, [(wc.write_collection(v, ent, f, comp), stream) for f in variants])
    plain = lambda f: [(fl, [struct.unpack('>H', i[1:])[0] if isinstance(i, bytes) else i for i in idx]) for fl, idx in f]   # noqa: E731
    for f, (rc, out) in zip(variants, got):
        assert rc == 0
        assert out == wc.assemble_collection(v, tables, plain(f))
    assert len(parts) == len(ent)


def test_batch_plan_mixes_single_fonts_and_collections(driver, tmp_path):
    singles = [(data, _oracle.decode(wf.parse(data)[2])) for name, data, sfnt, _, _ in wf.golden_files() if sfnt is not None]
    colls = [(woff2, _stream_of(woff2)) for _, woff2, _ in wc.golden_files()]
    assert len(singles) == 2 and len(colls) == 3
    mixed = [singles[0], colls[1], colls[2], singles[1], colls[0]]
    out = _run(driver, 'batch', _records(tmp_path, mixed)).split()
    assert out[:6] == ['batch', 'files', '5', 'collections', '3', 'orders'] and int(out[6]) >= 10


def test_host_parser_survives_damaged_collections(driver, tmp_path):
    """Every truncation, every bit of the CollectionHeader (and of numTables and
    totalCompressedSize), every 255UInt16 of it set to some 20 boundary values, written in its
    other forms (which must give the same TTC) and cut to a lone lead byte, and FUZZ_DOUBLES
    random double edits, of the three golden collections: 43,886 damaged files when this was
    written, 1,426 (3.2 %) accepted -- an index that names another table the font does not list
    yet, a flavor bit, a smaller totalCompressedSize (the program gets the stream apart), another
    encoding of the same value.  The program itself exits non-zero on any accepted file whose
    sources leave the stream, whose TTC header, directories and tables overlap or leave the
    announced size, or whose records are not strictly sorted by tag and at written tables."""
    src = _records(tmp_path, [(woff2, _stream_of(woff2)) for _, woff2, _ in wc.golden_files()])
    out = _run(driver, 'fuzz', src, FUZZ_SEED, FUZZ_DOUBLES).split()
    assert out[0] == 'damaged' and out[2] == 'accepted' and out[4] == 'rejected' and out[6] == 'same'
    damaged, accepted, rejected, same = int(out[1]), int(out[3]), int(out[5]), int(out[7])
    print('damaged %d accepted %d rejected %d same %d' % (damaged, accepted, rejected, same))
    assert damaged >= 20000 and accepted + rejected == damaged
    assert accepted > 0 and rejected > 0 and same > 0


def test_host_assembly_agrees_with_the_python_assembler(driver, tmp_path):
    """the kernel-alone cases of the GPU test, as collections whose tables all have the null transform"""
    cases = wc.kernel_cases()
    pairs = []
    for _, version, tables, fonts, _ in cases:
        ent = [[tag, 3 if tag in (b'glyf', b'loca') else 0, len(data), None] for tag, data in tables]
        pairs.append((wc.write_collection(version, ent, fonts, b''), b''.join(data for _, data in tables)))
    got = _assemble(driver, tmp_path, pairs)
    for (name, version, tables, fonts, _), (rc, out) in zip(cases, got):
        assert rc == 0, name
        assert out == wc.assemble_collection(version, tables, fonts), name
