"""woff2_encode / woff2_encode_batch over OpenType collections on the GPU
(brotli-lib_amd/csrc/woff2_write.hip, woff2_write_ttc.h): the compare kernel alone finds every
difference at every alignment; the files written for the golden TTCs and the hand-built ones say
what the Python statement of the rules says (tests/_woff2_collection_write.py) in every byte but
the Brotli stream, whose decoded bytes are the expected stream, and decode to the expected TTC;
tables are shared by content whatever the checkSum fields say; a batch gives per slot what the solo
call gives."""
import os
import shutil
import struct
import subprocess

import pytest

import _woff2_collection as wc
import _woff2_collection_write as cw
import _woff2_file as wf
import _woff2_write as ww
import brotli_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q5 = {'quality': 5, 'lgwin': 18}   # (where the Brotli bits are not what is looked at)
_memo = {}


def _tglyf(font):
    if ('g', font) not in _memo:
        _memo[('g', font)] = brotli_amd.woff2_transform_glyf(font)
    return _memo[('g', font)]


def _thmtx(font):
    if ('h', font) not in _memo:
        _memo[('h', font)] = brotli_amd.woff2_transform_hmtx(font)
    return _memo[('h', font)]


def _reconstruct(tglyf):
    if ('r', tglyf) not in _memo:
        _memo[('r', tglyf)] = brotli_amd.woff2_reconstruct_glyf(tglyf)
    return _memo[('r', tglyf)]


def _expected(ttc, transforms=3):
    return cw.expected(ttc, transforms, None, _tglyf, _thmtx)


def _solo(font, options=None):
    try:
        return brotli_amd.woff2_encode(font, options)
    except brotli_amd.BrotliError as e:
        return e.code


def _split(file, e):
    """(the bytes in front of the Brotli stream, the decoded stream) of a file, its length, padding
    and sizes checked against the expectation"""
    comp = struct.unpack('>L', file[20:24])[0]
    prefix = e.prefix(comp)
    assert file[:len(prefix)] == prefix
    assert len(file) == (len(prefix) + comp + 3) & ~3 and not any(file[len(prefix) + comp:])
    return prefix, brotli_amd.brotliDecode(file[len(prefix):len(prefix) + comp])


def _check(ttc, file, transforms, name):
    e = _expected(ttc, transforms)
    _, stream = _split(file, e)
    assert stream == e.stream, name
    out = brotli_amd.woff2_decode(file)
    assert out == cw.decoded(e, _reconstruct), name
    # every member's tables are the input member's, but for head's bytes 8..11 and flags bit 11 (and
    # glyf / loca, which come back normalised: they are the expectation's above)
    assert wc.read_ttc(out)[0] == e.version
    for m, (flavor, recs) in enumerate(cw.records(ttc)[1]):
        mine = wc.member_tables(out, m)
        assert wc.read_ttc(out)[1][m][0] == flavor and sorted(mine) == sorted(r[0] for r in recs), (name, m)
        for tag, _, off, n in recs:
            want, got = ttc[off:off + n], mine[tag]
            if tag == b'head' and n >= 12:   # (the decoder stores a checkSumAdjustment from 12 bytes on; the writer's fix from 18)
                want, got = [h[:8] + h[12:16] + bytes([x | 8 for x in h[16:17]]) + h[17:] for h in (want, got)]
            if tag not in (b'glyf', b'loca') or not transforms & 1:
                assert got == want, (name, m, tag)
    return e


# ---------------------------------------------------------------- the compare kernel alone
def test_tables_equal_kernel():
    blob = wf._blob
    pairs, mis_a, mis_b, want = [], [], [], []
    for n in (0, 1, 15, 16, 17, 4096, 4097, 3 * 4096 + 1):
        a = blob(n, n % 251)
        edits = [None] + ([[0], [n - 1]] if n else [])
        for tile in (4096, 8192, 3 * 4096):
            if n > tile:
                edits += [[tile - 1], [tile]]
            elif n == tile:
                edits += [[tile - 1]]
        for ma in (0, 7, 15):
            for mb in (0, 7, 15):
                for edit in edits:
                    b = bytearray(a)
                    for at in edit or []:
                        b[at] ^= 0x10
                    pairs.append((a, bytes(b)))
                    mis_a.append(ma)
                    mis_b.append(mb)
                    want.append(edit is None)
    a = blob(4097, 3)
    for ma in range(16):   # every misalignment of one side against another of the other
        for b, equal in ((a, True), (a[:-1] + bytes([a[-1] ^ 1]), False)):
            pairs.append((a, b))
            mis_a.append(ma)
            mis_b.append((5 * ma + 3) & 15)
            want.append(equal)
    assert len(pairs) >= 300   # one launch
    assert brotli_amd.debug_tables_equal(pairs, mis_a, mis_b) == want
    assert brotli_amd.debug_tables_equal(pairs[:5]) == want[:5]
    assert brotli_amd.debug_tables_equal([]) == []
    with pytest.raises(brotli_amd.BrotliError) as err:
        brotli_amd.debug_tables_equal([(b'ab', b'abc')])
    assert err.value.code == wf.MIB_E_INVALID_ARG
    try:
        brotli_amd.default_profiling(True)
        brotli_amd.debug_tables_equal(pairs[:9])
        assert brotli_amd.default_kernel_times()['w2enc_same'][1] == 1
    finally:
        brotli_amd.default_profiling(False)


# ---------------------------------------------------------------- whole files
def _collections():
    return [(name, ttc) for name, _, ttc in wc.golden_files()] + cw.hand_built()


@pytest.mark.parametrize('name', [name for name, _ in _collections()])
def test_collection_files(name):
    ttc = dict(_collections())[name]
    e = _check(ttc, brotli_amd.woff2_encode(ttc, Q5), 3, name)
    if name == 'ttc-shared-glyf':   # what the decoder's golden file says, entry for entry
        _, gent, gfonts, _ = wc.parse_collection(wc.golden_file(name)[0])
        assert sorted(map(tuple, e.entries)) == sorted(map(tuple, gent)) and len(e.fonts) == len(gfonts)
    if name in ('ttc-shared-glyf', 'ttc-two-glyf'):
        # these are what the decoder reconstructs, so normalised: glyf and loca come back as they went in, too
        out = brotli_amd.woff2_decode(brotli_amd.woff2_encode(ttc, Q5))
        for m in range(len(cw.records(ttc)[1])):
            a, b = wc.member_tables(ttc, m), wc.member_tables(out, m)
            assert a[b'glyf'] == b[b'glyf'] and a[b'loca'] == b[b'loca'], (name, m)


def test_options_choose_the_transforms():
    hand = dict(_collections())
    for name in ('three-members', 'ttc-two-glyf', 'two-hmtx-one-pair'):
        ttc = hand[name]
        e = _check(ttc, brotli_amd.woff2_encode(ttc, dict(Q5, transformGlyf=False)), 0, name)
        assert set(e.state) == {'plain'}
        e = _check(ttc, brotli_amd.woff2_encode(ttc, dict(Q5, transformHmtx=False)), 1, name)
        assert 'hmtx' not in e.state and 'glyf' in e.state
    ttc = hand['ttc-shared-glyf']
    _check(ttc, brotli_amd.woff2_encode(ttc), 3, 'defaults')   # quality 11, lgwin 22
    for options in ({'transforms': 4}, {'transforms': 0x80000001}):
        assert _solo(ttc, options) == wf.MIB_E_INVALID_ARG


def test_tables_are_shared_by_content():
    one = dict(cw.hand_built())['one-member']
    same, other = cw.two_copies(), cw.two_copies(True)
    f_same, f_other = brotli_amd.woff2_encode(same, Q5), brotli_amd.woff2_encode(other, Q5)
    e_same, e_other = _check(same, f_same, 3, 'two-copies'), _check(other, f_other, 3, 'one-name-byte')
    assert len(e_same.entries) == 7 and e_same.fonts[0][1] == e_same.fonts[1][1] == list(range(7))
    assert len(e_other.entries) == len(e_same.entries) + 1
    assert struct.unpack('>H', f_same[12:14])[0] == 7 and struct.unpack('>H', f_other[12:14])[0] == 8
    assert len(one) < len(same)
    # wrong checkSum fields: all zero (every table of a tag and length is compared: the same file), and
    # all different (nothing is compared, nothing is shared by content: another, correct file)
    zero = cw.two_copies(check=lambda data: 0)
    e = _check(zero, brotli_amd.woff2_encode(zero, Q5), 3, 'checksums-zero')
    assert e.entries == e_same.entries and e.fonts == e_same.fonts
    count = [0]

    def unique(data):
        count[0] += 1
        return count[0]
    apart = cw.two_copies(check=unique)
    assert not cw.candidates(apart)
    e = _check(apart, brotli_amd.woff2_encode(apart, Q5), 3, 'checksums-unique')
    assert len(e.entries) == 14
    # a checkSum that groups tables of different bytes: compared, found different, kept apart
    seven = cw.two_copies(True, check=lambda data: 7)
    e = _check(seven, brotli_amd.woff2_encode(seven, Q5), 3, 'checksums-seven')
    assert len(e.entries) == 8


def test_launches():
    """one compare launch for all collections of a call; none without candidates, none for single fonts"""
    shared = dict(cw.hand_built())['two-members-shared-head-v2']
    single = cw.member_sfnt(shared, 0)

    def times(fonts):
        try:
            brotli_amd.default_profiling(True)
            brotli_amd.woff2_encode_batch(fonts, Q5)
            return brotli_amd.default_kernel_times()
        finally:
            brotli_amd.default_profiling(False)
    t = times([cw.two_copies(), single, cw.two_copies(True)])
    assert t['w2enc_same'][1] == 1 and t['w2enc_pack'][1] == 1
    assert 'w2enc_same' not in times([shared, single])
    assert 'w2enc_same' not in times([single, single])


def test_rejections_and_statuses():
    for name, ttc in cw.rejected_collections():
        if len(ttc) > (1 << 20) + 4096:   # (16 MiB inputs: the host program's, tests/test_woff2_write_ttc_host.py)
            continue
        for options in (None, {'transformGlyf': False}):
            assert _solo(ttc, options) == wf.MIB_E_INVALID_ARG, name
    for name, ttc in cw.glyf_needs_collections():
        assert _solo(ttc) == wf.MIB_E_INVALID_ARG, name
        assert isinstance(_solo(ttc, dict(Q5, transformGlyf=False)), bytes), name   # stored as they are
    bad = cw.malformed_glyph_collection()
    assert _solo(bad, Q5) == wf.MIB_E_INVALID_ARG   # found on the device
    _check(bad, brotli_amd.woff2_encode(bad, dict(Q5, transformGlyf=False)), 0, 'malformed-glyph-stored')


def test_batch_in_groups():
    hand = dict(_collections())
    single = ww.golden_cases()[1][1]
    bad_glyph = cw.malformed_glyph_collection()
    rejected = cw.rejected_collections()[8][1]
    twice = hand['three-members']
    fonts = [twice, single, rejected, cw.two_copies(), hand['ttc-two-glyf'], bad_glyph, single, b'', twice,
             ww.rejected_fonts()[4][1], cw.two_copies(True), hand['65-members']]
    solo = [_solo(f, Q5) for f in fonts]
    assert [i for i, s in enumerate(solo) if not isinstance(s, bytes)] == [2, 5, 7, 9]
    results = {}
    try:
        for budget in (0, 40 * 1024, 1):   # one group; several; a font each
            brotli_amd.force_woff2_group_bytes(budget)
            results[budget] = brotli_amd.woff2_encode_batch(fonts, Q5)
    finally:
        brotli_amd.force_woff2_group_bytes(0)
    for budget, out in results.items():
        assert len(out) == len(fonts)
        for i, (s, b) in enumerate(zip(solo, out)):
            if not isinstance(s, bytes):
                assert isinstance(b, brotli_amd.BrotliError) and b.code == s, (budget, i)
                continue
            assert isinstance(b, bytes), (budget, i, b)
            # every byte but the stream: the header but its two sizes, and everything up to the stream
            assert b[:8] == s[:8] and b[12:20] == s[12:20] and b[24:48] == s[24:48], (budget, i)
            if s[4:8] == b'ttcf':
                e = _expected(fonts[i])
                ps, ds = _split(s, e)
                pb, db = _split(b, e)
                assert ps[48:] == pb[48:] and ds == db, (budget, i)
            else:
                assert wf.parse(b)[:2] == wf.parse(s)[:2], (budget, i)
                assert brotli_amd.brotliDecode(wf.parse(b)[2]) == brotli_amd.brotliDecode(wf.parse(s)[2]), (budget, i)
            assert brotli_amd.woff2_decode(b) == brotli_amd.woff2_decode(s), (budget, i)


def test_a_shared_pair_is_smaller_than_its_members_files():
    ttc, members = cw.shared_glyf_pair()
    for options in (Q5, None):
        whole = brotli_amd.woff2_encode(ttc, options)
        parts = brotli_amd.woff2_encode_batch(members, options)
        assert len(whole) < sum(len(p) for p in parts), options
    e = _check(ttc, whole, 3, 'shared-pair')
    assert [x[0] for x in e.entries].count(b'glyf') == 1


def test_python_round_trip():
    _, ttc = wc.golden_file('ttc-two-glyf')
    file = brotli_amd.woff2_encode(bytearray(ttc))
    assert file[:8] == b'wOF2ttcf'
    back = brotli_amd.woff2_decode(file)
    assert len(back) == len(ttc) and wc.read_ttc(back)[0] == wc.V2
    assert brotli_amd.woff2_decode(brotli_amd.woff2_encode(back)) == back


def test_node_woff2_encode_collection():
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'woff2_encode_collection_test.js')], capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
