"""The WOFF2 writer's collection plan without a GPU: brotli-lib_amd/csrc/woff2_write_ttc.h, built as
host code with AddressSanitizer and UBSan into a stand-alone program
(tests/woff2_write_ttc_host_main.cpp), gives for the golden TTCs and the hand-built ones the bytes
that the Python statement of the rules gives (tests/_woff2_collection_write.py), rejects every item
of its rejection list with its number, takes damaged collections without a report or a broken
plan, and writes only containers that the decoder's host plan (woff2_file.h) assembles into the
expected TTC.  The compare's answers are input here (there is no device); the transformed tables
are fontTools'."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

import _woff2_collection as wc
import _woff2_collection_write as cw
import _woff2_file as wf
import _woff2_reconstruct as w2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, wf.HERE)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('woff2_write_ttc') / 'woff2_write_ttc_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'woff2_write_ttc_host_main.cpp'), '-o', exe], check=True)
    return exe


@pytest.fixture(scope='module')
def ft():
    """fontTools' transforms of a member and its reconstruction of a transformed glyf, cached"""
    pytest.importorskip('fontTools')
    import make_golden
    import make_reconstruct_golden as rec
    cache = {}

    def memo(kind, f):
        def g(font):
            if (kind, font) not in cache:
                cache[(kind, font)] = f(font)
            return cache[(kind, font)]
        return g

    by_tglyf = {}

    def tglyf(font):
        # (the transform reads numGlyphs + 1 loca entries; fontTools wants no more in the table)
        t = wf.sfnt_tables(font)
        ng, long_loca = struct.unpack('>H', t[b'maxp'][4:6])[0], struct.unpack('>h', t[b'head'][50:52])[0] != 0
        t[b'loca'] = t[b'loca'][:(ng + 1) * (4 if long_loca else 2)]
        font = wf.assemble(struct.unpack('>L', font[:4])[0], sorted(t.items()))
        t = make_golden.transform(font)
        by_tglyf[t] = font
        return t

    def reconstruct(t):
        return rec.reconstruct(by_tglyf[t], t)[:2]
    return memo('g', tglyf), memo('h', make_golden.transform_hmtx), reconstruct


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _list(tables):
    return b''.join(struct.pack('<LL', i, len(b)) + b for i, b in tables)


def _pack(exe, tmp_path, cases):
    """[(answer, directory + CollectionHeader, header, stream, the TTC read back)] over
    [(ttc, transforms, differ, [(entry, tglyf)], [(entry, thmtx)], compressed size)]"""
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        for ttc, transforms, differ, tglyf, thmtx, comp in cases:
            f.write(w2.record(ttc) + w2.record(bytes([transforms])) + w2.record(bytes(differ)) + w2.record(_list(tglyf)) +
                    w2.record(_list(thmtx)) + w2.record(struct.pack('<L', comp)))
    assert _run(exe, 'pack', src, dst).strip() == 'packed %d' % len(cases)
    with open(dst, 'rb') as f:
        b = f.read()
    recs, at = [], 0
    while at < len(b):
        n = struct.unpack('<L', b[at:at + 4])[0]
        recs.append(b[at + 4:at + 4 + n])
        at += 4 + n
    assert len(recs) == 5 * len(cases)
    return [(struct.unpack('<l', recs[i])[0],) + tuple(recs[i + 1:i + 5]) for i in range(0, len(recs), 5)]


def _case(e, ttc, transforms, comp):
    return (ttc, transforms, [1 if d else 0 for d in e.differ], [(i, p) for i, (p, s) in enumerate(zip(e.parts, e.state)) if s == 'glyf'],
            [(i, p) for i, (p, s) in enumerate(zip(e.parts, e.state)) if s == 'hmtx'], comp)


def _collections():
    return [(name, ttc) for name, _, ttc in wc.golden_files()] + cw.hand_built()


def test_the_hand_built_collections_are_what_they_are_named():
    got = dict(cw.hand_built())
    counts = {name: len(cw.records(ttc)[1]) for name, ttc in got.items()}
    assert {1, 2, 3, 65} <= set(counts.values())
    assert {cw.records(ttc)[0] for ttc in got.values()} == {wc.V1, wc.V2}
    assert len(cw.candidates(got['two-copies'])) == 7 and not cw.candidates(got['three-members'])
    assert all(len(ttc) < 64 * 1024 for ttc in got.values())


def test_plan_gives_the_python_statement(driver, tmp_path, ft):
    tglyf, thmtx, reconstruct = ft
    keys, cases, want = [], [], []
    for name, ttc in _collections():
        for transforms in (3, 1, 0):
            e = cw.expected(ttc, transforms, None, tglyf, thmtx)
            keys.append((name, transforms))
            cases.append(_case(e, ttc, transforms, 5))
            want.append(e)
    for key, e, (rc, between, header, stream, back) in zip(keys, want, _pack(driver, tmp_path, cases)):
        assert rc == 0, key
        assert header + between == e.prefix(5), key
        assert stream == e.stream, key
        assert back == cw.decoded(e, reconstruct), key   # the decoder accepts the file, and what it makes of it
    # what the cases cover
    by = dict(zip(keys, want))
    e = by[('three-members', 3)]
    tags = [x[0] for x in e.entries]
    assert tags.count(b'glyf') == 2 and tags.count(b'loca') == 2 and tags.count(b'head') == 2 and b'DSIG' not in tags
    assert e.state.count('hmtx') == 0 and tags.count(b'hmtx') == 1   # one hmtx under two pairs: stored as it is
    assert by[('hmtx-under-two-hheas', 3)].state.count('hmtx') == 0 and by[('two-hmtx-one-pair', 3)].state.count('hmtx') == 2
    assert by[('two-members-shared-head-v2', 3)].state.count('hmtx') == 1 and by[('ttc-shared-glyf', 3)].state.count('hmtx') == 1
    assert len(by[('two-copies', 3)].entries) == 7
    assert len(by[('two-copies-one-name-byte', 3)].entries) == 8
    assert by[('ttc-two-glyf', 0)].state.count('plain') == len(by[('ttc-two-glyf', 0)].state)


def test_the_compares_answers_decide(driver, tmp_path, ft):
    """the same TTC under other answers: every candidate different (no table shared by content), and
    only glyf different (the pair is written twice though the locas are equal)"""
    tglyf, thmtx, reconstruct = ft
    ttc = cw.two_copies()
    cand = cw.candidates(ttc)
    flat = [r for _, recs in cw.records(ttc)[1] for r in recs]
    only_glyf = [flat[a][0] == b'glyf' for a, _ in cand]
    assert sum(only_glyf) == 1
    cases, want = [], []
    for differ in ([True] * len(cand), only_glyf, [False] * len(cand)):
        e = cw.expected(ttc, 3, differ, tglyf, thmtx)
        want.append(e)
        cases.append(_case(e, ttc, 3, 0))
    assert [len(e.entries) for e in want] == [14, 9, 7]
    for e, (rc, between, header, stream, back) in zip(want, _pack(driver, tmp_path, cases)):
        assert rc == 0 and header + between == e.prefix(0) and stream == e.stream
        assert back == cw.decoded(e, reconstruct)


def test_plan_rejects_the_list(driver, tmp_path):
    cases = cw.rejected_collections()
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(10, 20))
    for transforms in (0, 3):
        got = _pack(driver, tmp_path, [(ttc, transforms, b'', [], [], 0) for _, ttc in cases])
        for (name, _), (rc, between, header, stream, back) in zip(cases, got):
            assert rc == int(name.split('-')[0]), name
            assert between == header == stream == back == b'', name
    # 16's counterpart: the same lengths at one offset count once
    ttc = cw.same_length_accepted()
    e = cw.expected(ttc, 0)
    (rc, between, header, stream, back), = _pack(driver, tmp_path, [_case(e, ttc, 0, 0)])
    assert rc == 0 and header + between == e.prefix(0) and len(stream) == 16 << 20 and len(e.entries) == 1


def test_plan_rejects_what_the_glyf_transform_needs(driver, tmp_path, ft):
    tglyf, thmtx, _ = ft
    cases = cw.glyf_needs_collections()
    assert len(cases) == 5
    got = _pack(driver, tmp_path, [(ttc, 3, b'', [], [], 0) for _, ttc in cases])
    for (name, _), g in zip(cases, got):
        assert g[0] == 20, name
    # with the transform off the same collections are stored as they are
    want = [cw.expected(ttc, 0) for _, ttc in cases]
    got = _pack(driver, tmp_path, [_case(e, ttc, 0, 0) for e, (_, ttc) in zip(want, cases)])
    for (name, _), e, g in zip(cases, want, got):
        assert g[0] == 0 and g[1] == e.between() and g[3] == e.stream, name


def test_plan_survives_damaged_collections(driver, tmp_path):
    """Every truncation up to the last directory's end, every bit of the TTC header and the
    directories, and every member offset, table offset and table length set to some 56 values, of
    hand-built collections of two and three members (shared and unshared tables, a DSIG, version
    2.0).  The program itself exits non-zero on a plan whose sources leave the input, whose stream
    pieces overlap or leave stream_len, whose members' indices are not below the entry count, or
    whose container the decoder's parse refuses, and runs ttc_host_pack over every accepted plan
    under the sanitizers."""
    src = str(tmp_path / 'in.bin')
    hand = dict(cw.hand_built())
    with open(src, 'wb') as f:
        for name in ('two-members-shared-head-v2', 'three-members', 'two-copies-one-name-byte'):
            f.write(w2.record(hand[name]))
    out = _run(driver, 'fuzz', src).split()
    assert out[0] == 'damaged' and out[2] == 'accepted' and out[4] == 'rejected' and out[6] == 'why'
    damaged, accepted, rejected = int(out[1]), int(out[3]), int(out[5])
    print(' '.join(out))
    assert damaged >= 10000 and accepted + rejected == damaged
    assert accepted > 0 and rejected > damaged // 4
    why = [int(v) for v in out[7:]]
    assert len(why) == 20 and why[9] > 0 and why[10] > 0 and why[12] > 0   # items 10, 11, 13
