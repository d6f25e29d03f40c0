"""Shared by the WOFF2 collection tests and tests/golden/woff2/make_collection_golden.py: the
container of a font collection (flavor ttcf: W3C WOFF2 section 4.2) in pure Python -- writer and
parser --, the TTC assembler that states the layout rules of DESIGN.md 4c "A font collection"
(the expectation of both the host and the device assembly), a TTC reader, the fixtures of
tests/golden/woff2/collection_golden.json, the collections that must be rejected (items 14 - 20
of the rejection list; item 21 cannot be reached from a file, see rejected_collections) and the
assembly kernels' cases."""
import base64
import json
import os
import struct

import _woff2_file as wf

TTCF = 0x74746366
V1, V2 = 0x00010000, 0x00020000
TRUE, OTTO = 0x74727565, 0x4F54544F   # the flavors 'true' and 'OTTO'


# ---------------------------------------------------------------- 255UInt16
def u255(v):
    """the shortest encoding"""
    if v < 253:
        return bytes([v])
    if v < 506:
        return bytes([255, v - 253])
    if v < 762:
        return bytes([254, v - 506])
    return bytes([253]) + struct.pack('>H', v)


def u255_word(v):
    """the three-byte encoding, canonical or not"""
    return bytes([253]) + struct.pack('>H', v)


def _read255(b, at):
    c = b[at]
    if c < 253:
        return c, at + 1
    if c == 253:
        return struct.unpack('>H', b[at + 1:at + 3])[0], at + 3
    return (506 if c == 254 else 253) + b[at + 1], at + 2


# ---------------------------------------------------------------- the container
def write_collection(version, entries, fonts, compressed, known=True, num_fonts=None):
    """A .woff2 file of flavor ttcf.  entries: as _woff2_file.write takes them, every table of
    every font once; fonts: [(flavor, [index, ...])] or [(flavor, [index, ...], numTables)]; an
    index, a numTables and num_fonts may be raw bytes (any 255UInt16 encoding, or a broken one)."""
    raw = lambda v: v if isinstance(v, bytes) else u255(v)   # noqa: E731
    directory = wf.write(TTCF, entries, b'', known)[48:]
    c = struct.pack('>L', version) + raw(len(fonts) if num_fonts is None else num_fonts)
    for font in fonts:
        flavor, idx = font[0], font[1]
        c += raw(font[2] if len(font) > 2 else len(idx)) + struct.pack('>L', flavor) + b''.join(raw(i) for i in idx)
    total = 48 + len(directory) + len(c) + len(compressed)
    head = struct.pack('>4sLLHHLLHHLLLLL', b'wOF2', TTCF, total, len(entries), 0, 0, len(compressed), 1, 0, 0, 0, 0, 0, 0)
    return head + directory + c + compressed


def parse_collection(data):
    """(version, entries, [(flavor, [index, ...])], compressed stream) of a well-formed file"""
    sig, flavor, length, k, _, _, comp = struct.unpack('>4sLLHHLL', data[:24])
    assert sig == b'wOF2' and flavor == TTCF and length == len(data)
    at = 48
    entries = []
    for _ in range(k):
        flags = data[at]
        at += 1
        if flags & 63 == 63:
            tag = data[at:at + 4]
            at += 4
        else:
            tag = wf.KNOWN_TAGS[flags & 63]
        orig, at = wf._read_base128(data, at)
        tlen = None
        if wf.is_transformed(tag, flags >> 6):
            tlen, at = wf._read_base128(data, at)
        entries.append([tag, flags >> 6, orig, tlen])
    version = struct.unpack('>L', data[at:at + 4])[0]
    nf, at = _read255(data, at + 4)
    fonts = []
    for _ in range(nf):
        nt, at = _read255(data, at)
        fl = struct.unpack('>L', data[at:at + 4])[0]
        at += 4
        idx = []
        for _ in range(nt):
            i, at = _read255(data, at)
            idx.append(i)
        fonts.append((fl, idx))
    assert at + comp <= len(data)
    return version, entries, fonts, data[at:at + comp]


def cut_list(entries, stream):
    """[each entry's bytes in the decompressed stream] (tags repeat in a collection)"""
    out, at = [], 0
    for n in wf.stream_lengths(entries):
        out.append(stream[at:at + n])
        at += n
    assert at == len(stream)
    return out


# ---------------------------------------------------------------- the TTC's layout
def assemble_collection(version, tables, fonts):
    """The TTC of tables = [(tag, bytes)] (the collection's directory, in its order) and fonts =
    [(flavor, [index, ...])]: header ('ttcf', version, numFonts, the offset tables' offsets, three
    zero words more for version 2.0), the members' directories back to back (records sorted by
    tag, offsets file-relative), then every table that a font lists, once, in the directory's
    order, at 4-byte boundaries and zero-padded.  A table has one checksum (head's with bytes
    8..11 as zero) whoever lists it; a head's bytes 8..11 become 0xB1B0AFBA - (the sum of the
    last font that lists it: its offset table, its records, its tables' checksums)."""
    nf = len(fonts)
    at = 12 + 4 * nf + (12 if version == V2 else 0)
    dir_off = []
    for _, idx in fonts:
        dir_off.append(at)
        at += 12 + 16 * len(idx)
    written = {i for _, idx in fonts for i in idx}
    recs, body = {}, bytearray()
    for i, (tag, data) in enumerate(tables):
        if i not in written:
            continue
        data = bytes(data)
        if tag == b'head' and len(data) >= 12:
            data = data[:8] + bytes(4) + data[12:]
        recs[i] = (tag, wf.checksum(data), at + len(body), len(data))
        body += data + b'\0' * (-len(data) % 4)
    out = bytearray(struct.pack('>LLL', TTCF, version, nf) + struct.pack('>%dL' % nf, *dir_off))
    if version == V2:
        out += bytes(12)
    adjust = {}
    for flavor, idx in fonts:
        k = len(idx)
        sel = 0
        while (2 << sel) <= k:
            sel += 1
        d = struct.pack('>LHHHH', flavor, k, ((1 << sel) * 16) & 0xFFFF, sel & 0xFFFF, (k * 16 - (1 << sel) * 16) & 0xFFFF)
        for tag, cs, off, length in sorted(recs[i] for i in idx):
            d += tag + struct.pack('>LLL', cs, off, length)
        out += d
        total = wf.checksum(d) + sum(recs[i][1] for i in idx)
        for i in idx:
            if recs[i][0] == b'head' and recs[i][3] >= 12:
                adjust[recs[i][2]] = (wf.HEAD_MAGIC - total) & 0xFFFFFFFF   # (a later font's replaces it)
    out += body
    for off, v in adjust.items():
        out[off + 8:off + 12] = struct.pack('>L', v)
    return bytes(out)


def read_ttc(ttc):
    """(version, [(flavor, [(tag, checksum, offset, length)])]) of a TTC"""
    sig, version, nf = struct.unpack('>LLL', ttc[:12])
    assert sig == TTCF
    fonts = []
    for off in struct.unpack('>%dL' % nf, ttc[12:12 + 4 * nf]):
        flavor, k = struct.unpack('>LH', ttc[off:off + 6])
        fonts.append((flavor, [struct.unpack('>4sLLL', ttc[off + 12 + 16 * r:off + 28 + 16 * r]) for r in range(k)]))
    return version, fonts


def member_tables(ttc, member):
    """{tag: bytes} of one font of a TTC"""
    return {tag: ttc[off:off + length] for tag, _, off, length in read_ttc(ttc)[1][member][1]}


# ---------------------------------------------------------------- fixtures
def golden():
    with open(os.path.join(wf.HERE, 'collection_golden.json')) as f:
        return json.load(f)


def golden_files():
    """[(name, .woff2 bytes, TTC bytes)]"""
    return [(name, base64.b64decode(fx['woff2']), base64.b64decode(fx['ttc']))
            for name, fx in sorted(golden()['files'].items())]


def golden_file(name):
    fx = golden()['files'][name]
    return base64.b64decode(fx['woff2']), base64.b64decode(fx['ttc'])


def rejected_collections():
    """[(id, file, the golden's name)]: every one is MIB_E_INVALID_ARG, decided by the parser: each
    is a golden collection with one edit, its Brotli stream left as it was.  The ids' numbers are the items of
    the rejection list.  Item 21 (a TTC whose offsets leave 32 bits) has no file:
    the tables of a stream of at most 256 MiB, each written once, cannot get there; the stand-alone
    host program puts the rule to a hand-made plan instead."""
    shared = parse_collection(golden_file('ttc-shared-glyf')[0])
    two = parse_collection(golden_file('ttc-two-glyf')[0])
    cases = []

    def add(name, base, version=None, entries=None, fonts=None, comp=None, **kw):
        v, e, f, c = base
        file = write_collection(v if version is None else version, e if entries is None else entries,
                                f if fonts is None else fonts, c if comp is None else comp, **kw)
        cases.append((name, file, 'ttc-shared-glyf' if base is shared else 'ttc-two-glyf'))

    def find(base, tag, nth=0):
        return [i for i, e in enumerate(base[1]) if e[0] == tag][nth]

    def relist(base, member, change):
        """the fonts with one member's index list passed through change()"""
        return [(fl, change(list(idx)) if m == member else idx) for m, (fl, idx) in enumerate(base[2])]

    def without(*drop):
        return lambda idx: [i for i in idx if i not in drop]

    def swapped(a, b):
        return lambda idx: [b if i == a else i for i in idx]

    def retag(base, i, **kw):
        out = [list(e) for e in base[1]]
        for k, v in kw.items():
            out[i][('tag', 'version', 'orig', 'tlen').index(k)] = v
        return out

    k = len(shared[1])
    add('14-version-0', shared, version=0)
    add('14-version-3', shared, version=0x00030000)
    add('14-version-1-minor-1', shared, version=0x00010001)
    add('15-no-fonts', shared, fonts=[])
    add('15-font-without-tables', shared, fonts=shared[2] + [(V1, [])])
    add('16-index-at-numtables', shared, fonts=relist(shared, 1, swapped(find(shared, b'maxp'), k)))
    add('16-index-65535', shared, fonts=relist(shared, 0, swapped(find(shared, b'maxp'), 65535)))
    add('16-tag-twice-in-a-font', shared, fonts=relist(shared, 0, lambda idx: idx + [find(shared, b'name', 1)]))
    add('16-index-twice-in-a-font', shared, fonts=relist(shared, 1, lambda idx: idx + [find(shared, b'maxp')]))
    good = write_collection(*shared)
    cut_at = len(good) - len(shared[3]) - 3   # inside the last font's indices
    cut_file = bytearray(good[:cut_at])
    cut_file[8:12] = struct.pack('>L', cut_at)
    cut_file[20:24] = struct.pack('>L', 0)
    cases.append(('17-header-cut-short', bytes(cut_file), 'ttc-shared-glyf'))
    add('17-more-fonts-than-the-file-holds', shared, num_fonts=len(shared[2]) + 1)
    add('17-more-tables-than-the-font-lists', shared, fonts=shared[2][:1] + [shared[2][1] + (len(shared[2][1][1]) + 1,)])
    over = bytearray(good)
    over[20:24] = struct.pack('>L', len(shared[3]) + 1)
    cases.append(('17-compressed-size-past-the-file', bytes(over), 'ttc-shared-glyf'))
    g, loca, name0 = find(shared, b'glyf'), find(shared, b'loca'), find(shared, b'name')
    moved = [list(e) for e in shared[1]]
    moved[loca], moved[name0] = moved[name0], moved[loca]
    add('18-glyf-not-followed-by-loca', shared, entries=moved)
    add('18-loca-in-another-state', shared, entries=retag(shared, loca, version=3, orig=0, tlen=None))
    add('18-loca-without-glyf', shared, entries=retag(shared, g, tag=b'glyX', version=0, tlen=None))
    add('18-font-lists-glyf-alone', shared, fonts=relist(shared, 1, without(loca)))
    add('18-font-lists-loca-alone', shared, fonts=relist(shared, 0, without(g)))
    add('18-font-lists-another-pairs-loca', two, fonts=relist(two, 0, swapped(find(two, b'loca', 0), find(two, b'loca', 1))))
    hm, hh = find(shared, b'hmtx'), find(shared, b'hhea')
    add('19-hmtx-font-without-glyf', shared, fonts=relist(shared, 1, without(g, loca)))
    add('19-hmtx-font-without-hhea', shared, fonts=relist(shared, 0, without(hh)))
    add('19-hmtx-hhea-35-bytes', shared, entries=retag(shared, hh, orig=35))
    null = retag(shared, g, version=3, orig=shared[1][g][3], tlen=None)
    null[loca] = [b'loca', 3, 0, None]
    add('19-hmtx-glyf-null', shared, entries=null)
    # ttc-two-glyf: font 0 has the transformed hmtx; font 1 takes it too, beside its own glyf
    # pair (another glyf for the same entry), then beside font 0's pair but its own hhea
    hm0, hm1 = find(two, b'hmtx', 0), find(two, b'hmtx', 1)
    assert two[1][hm0][1] == 1 and two[1][hm1][1] == 0 and hm0 in two[2][0][1] and hm1 in two[2][1][1]
    add('19-hmtx-two-glyfs', two, fonts=relist(two, 1, swapped(hm1, hm0)))
    both = swapped(hm1, hm0)
    pair = lambda idx: swapped(find(two, b'loca', 1), find(two, b'loca', 0))(   # noqa: E731
        swapped(find(two, b'glyf', 1), find(two, b'glyf', 0))(both(idx)))
    add('19-hmtx-two-hheas', two, fonts=relist(two, 1, pair))
    # 17 fonts of 65,535 tables: 17 * (12 + 16 * 65535) bytes of directories, above 16 MiB
    add('20-directories-above-16-MiB', shared, fonts=[(V1, [bytes(65535)], u255(65535))] * 17)
    return cases


# ---------------------------------------------------------------- the assembly kernels' cases
def kernel_cases():
    """[(id, version, [(tag, bytes)], [(flavor, [index, ...])], misalign or None)]"""
    blob, head = wf._blob, wf._head
    c = []
    for n in (1, 2, 3, 65):   # header lengths 16, 20, 24, 272; more fonts than a wave has lanes
        tables = [(b'cmap', blob(21, 1))] + [(b'name', blob(5 + f, f)) for f in range(n)]
        c.append(('%d-fonts' % n, V1, tables, [(V1 if f % 2 == 0 else TRUE, [0, 1 + f]) for f in range(n)], None))
    tables = [(b'cmap', blob(21, 1)), (b'name', blob(9, 2)), (b'name', blob(10, 3))]
    c.append(('version-2', V2, tables, [(V1, [0, 1]), (TRUE, [0, 2])], None))
    c.append(('version-2-one-font', V2, tables[:2], [(V1, [1, 0])], None))
    for n in (1, 64, 65):
        tables = [(b'T%03d' % i, blob(3 * i + 1, i)) for i in range(n)] + [(b'post', blob(13, 7))]
        c.append(('member-of-%d-tables' % n, V1, tables, [(V1, list(range(n))), (V1, [n])], None))
    shared = [(b'cmap', blob(40, 1)), (b'gvar', blob(333, 2)), (b'name', blob(17, 3)), (b'name', blob(18, 4))]
    c.append(('shared-tables', V1, shared, [(V1, [0, 1, 2]), (V1, [0, 1, 3])], None))
    hd = head(54, 9)
    c.append(('shared-head', V1, shared + [(b'head', hd)], [(V1, [0, 1, 2, 4]), (V1, [0, 1, 3, 4]), (TRUE, [1, 3])], None))
    c.append(('shared-head-three-fonts', V2, shared + [(b'head', hd)], [(V1, [4, 0]), (V1, [4, 1, 2]), (TRUE, [3, 4])], [1, 13, 6, 15, 9]))
    c.append(('head-in-one-font', V1, shared + [(b'head', hd)], [(V1, [0, 1, 2]), (V1, [0, 1, 3, 4])], None))
    c.append(('head-per-font', V1, shared + [(b'head', hd), (b'head', head(54, 10))], [(V1, [0, 1, 2, 4]), (V1, [0, 1, 3, 5])], None))
    c.append(('head-11-bytes', V1, shared + [(b'head', head(11, 5))], [(V1, [0, 4]), (V1, [1, 4])], None))
    c.append(('head-12-bytes', V1, shared + [(b'head', head(12, 5))], [(V1, [0, 4]), (V1, [1, 4])], None))
    c.append(('empty-shared-table', V1, [(b'cvt ', b''), (b'name', blob(7, 1)), (b'name', blob(8, 2))],
              [(V1, [0, 1]), (V1, [0, 2])], None))
    c.append(('only-empty-tables', V1, [(b'cvt ', b''), (b'prep', b'')], [(V1, [0]), (V1, [1, 0])], None))
    c.append(('entry-no-font-lists', V1, [(b'cmap', blob(40, 1)), (b'DSIG', blob(100, 2)), (b'name', blob(17, 3)), (b'post', blob(3, 4))],
              [(V1, [0, 2]), (V1, [0, 3])], None))
    c.append(('first-and-last-entry-unlisted', V1, [(b'DSIG', blob(33, 2)), (b'cmap', blob(40, 1)), (b'junk', blob(5, 4))],
              [(V1, [1])], None))
    six = [(b'zzzz', blob(9, 1)), (b'maxp', blob(32, 2)), (b'cmap', blob(40, 3)), (b'OS/2', blob(96, 4)), (b'aaaa', blob(2, 5)),
           (b'maxp', blob(32, 6))]
    c.append(('listed-in-another-order', V1, six, [(V1, [4, 3, 2, 1, 0]), (TRUE, [5, 0, 4, 2])], None))
    for m in (0, 7, 15):
        c.append(('shared-tiles-plus-one-misalign-%d' % m, V1,
                  [(b'cmap', blob(7, 1)), (b'CFF ', blob(3 * 4096 + 1, 2)), (b'post', blob(9, 3)), (b'post', blob(10, 4))],
                  [(OTTO, [0, 1, 2]), (V1, [1, 3])], [3, m, 2, 5]))
    # 5 words of 0xFF sum past 2^32; 4100 bytes: across a tile as well; both tables in both fonts
    c.append(('sums-wrap', V1, [(b'cvt ', b'\xff' * 4100), (b'prep', b'\xff' * 19), (b'head', b'\xff' * 54)],
              [(0xFFFFFFFF, [0, 1, 2]), (0xFFFFFFFF, [2, 1, 0])], [9, 2, 0]))
    return c
