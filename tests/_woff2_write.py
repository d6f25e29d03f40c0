"""Shared by the WOFF2 writer's tests: the golden files' source fonts, what the file of a font has
to be but for its Brotli bits (brotli-lib_amd/csrc/woff2_write.h, DESIGN.md 4c "Writing a file"),
the fonts that must be rejected, and the hand-built fonts of the copy kernel's edges."""
import base64
import os
import struct

import _inputs
import _oracle
import _woff2_file as wf

GLYF, HMTX = 1, 2
BENCH = os.path.join(_inputs.GOLDEN, 'bench')
_cache = {}


def _source(name):
    if name not in _cache:
        if name.startswith('synthetic'):
            _cache[name] = base64.b64decode(wf.golden()['synthetic'][name]['sfnt'])
        elif name == 'enc-var-ttf':
            with open(os.path.join(BENCH, 'enc-var-ttf.br'), 'rb') as f:
                _cache[name] = _oracle.decode(f.read())
        else:
            with open(os.path.join(BENCH, name + '.bin'), 'rb') as f:
                _cache[name] = f.read()
    return _cache[name]


def golden_cases():
    """[(name, source sfnt, golden .woff2, transforms, sfnt size, sfnt sha256)]: the seven files
    fontTools wrote, each with the transforms of its variant"""
    if 'cases' not in _cache:
        out = []
        for name, data, _, size, sha in wf.golden_files():
            hm = name.endswith('-hmtx')
            src = _source(name if name.startswith('synthetic') else (name[:-5] if hm else name))
            out.append((name, src, data, GLYF | (HMTX if hm else 0), size, sha))
        _cache['cases'] = out
    return _cache['cases']


def golden_stream(data):
    """(entries, the golden file's decompressed stream) -- decoded once per file"""
    key = ('stream', hash(data), len(data))
    if key not in _cache:
        _, ent, comp = wf.parse(data)
        _cache[key] = (ent, _oracle.decode(comp))
    return _cache[key]


def directory_bytes(data):
    """the bytes between a file's header and its compressed stream"""
    flavor, ent, comp = wf.parse(data)
    at = len(wf.write(flavor, ent, b''))
    assert data[at:at + len(comp)] == comp
    assert len(data) % 4 == 0 and len(data) - at - len(comp) < 4 and not any(data[at + len(comp):])   # zero padding to 4 bytes
    assert len(comp) == struct.unpack('>L', data[20:24])[0]
    return data[48:at]


def zero_head(ent, stream):
    """the stream with head's bytes 8..11 as zero (fontTools keeps the font's checkSumAdjustment)"""
    at = dict(zip([e[0] for e in ent], wf._offsets(ent)))
    if b'head' not in at:
        return stream
    h = at[b'head']
    return stream[:h + 8] + bytes(4) + stream[h + 12:]


def options(transforms, quality=None, lgwin=None):
    o = {'transformGlyf': bool(transforms & GLYF), 'transformHmtx': bool(transforms & HMTX)}
    if quality is not None:
        o['quality'] = quality
    if lgwin is not None:
        o['lgwin'] = lgwin
    return o


# ---------------------------------------------------------------- hand-built fonts
def sfnt(flavor, tables, gaps=None, num=None):
    """An sfnt of [(tag, bytes)] whose records stand in the list's order and point at data placed
    back to back with gaps[i] bytes of filler in front of table i (None: none, so offsets are
    unaligned wherever lengths are odd).  Checksums and search fields are zero: the writer reads
    neither."""
    k = len(tables)
    out = bytearray(struct.pack('>LHHHH', flavor, k if num is None else num, 0, 0, 0))
    at = 12 + 16 * k
    body = bytearray()
    for i, (tag, data) in enumerate(tables):
        g = gaps[i] if gaps is not None else 0
        body += b'\xEE' * g
        out += tag + struct.pack('>LLL', 0, at + len(body), len(data))
        body += data
    return bytes(out + body)


def expected_entries_and_stream(tables, glyf_transformed=False):
    """what the file of a font with no transformed table says: [[tag, version, orig, None]] and the
    stream, from [(tag, bytes)] in any order"""
    ent, stream = [], b''
    for tag, data in sorted(tables):
        if tag == b'DSIG':
            continue
        if tag == b'head' and len(data) >= 18:
            data = data[:8] + bytes(4) + data[12:16] + bytes([data[16] | (8 if glyf_transformed else 0)]) + data[17:]
        ent.append([tag, 3 if tag in (b'glyf', b'loca') else 0, len(data), None])
        stream += data
    return ent, stream


def total_sfnt_size(ent):
    return 12 + 16 * len(ent) + sum((e[2] + 3) & ~3 for e in ent)


def expected_prefix(flavor, ent, tables, comp_len):
    """header + directory of the file whose compressed stream has comp_len bytes: the length padded
    to 4 bytes, totalSfntSize from the origLengths, the version head's fontRevision (else 0.0)"""
    d = wf.write(flavor, ent, b'')[48:]
    head = dict(tables).get(b'head', b'')
    version = head[4:8] if len(head) >= 8 else bytes(4)
    total = (48 + len(d) + comp_len + 3) & ~3
    return struct.pack('>4sLLHHLL', b'wOF2', flavor, total, len(ent), 0, total_sfnt_size(ent), comp_len) + version + bytes(20) + d


def pack_cases():
    """[(id, sfnt, [(tag, bytes)])]: fonts without glyf, for the copy kernel's edges"""
    blob = wf._blob
    c = []
    sizes = (0, 1, 2, 3, 15, 16, 17, 33, 3 * 4096 + 1)
    tables = [(b'tb%02d' % i, blob(n, i + 1)) for i, n in enumerate(sizes)]
    c.append(('lengths', sfnt(0x4F54544F, tables), tables))
    for m in range(16):
        # the first table's data begins at 12 + 16 * 3 + gap: every misalignment of the source, while
        # the destinations' misalignments follow from the lengths
        tables = [(b'name', blob(33, m)), (b'post', blob(50, m + 16)), (b'cmap', blob(4096 + 7, m + 32))]
        c.append(('misalign-%d' % m, sfnt(0x00010000, tables, gaps=[(m + 4) & 15, m, 15 - m]), tables))
    tables = [(b'cmap', blob(40, 1)), (b'DSIG', blob(29, 2)), (b'post', blob(21, 3))]
    c.append(('dsig', sfnt(0x00010000, tables), tables))
    tables = [(b'Zzzz', blob(19, 4)), (b'cmap', blob(40, 1)), (b'abcd', blob(5, 2))]
    c.append(('unknown-tags', sfnt(0x00010000, tables), tables))
    head = blob(54, 9)
    head = head[:16] + bytes([head[16] & ~8]) + head[17:]
    assert head[8:12] != bytes(4)
    for name, t, gaps in (('head-first', [(b'head', head), (b'maxp', blob(32, 2)), (b'post', blob(21, 3))], None),
                          ('head-last', [(b'OS/2', blob(31, 2)), (b'cmap', blob(45, 3)), (b'head', head)], None),
                          ('head-middle', [(b'cmap', blob(45, 3)), (b'head', head), (b'post', blob(21, 3))], [1, 6, 3])):
        c.append((name, sfnt(0x00010000, t, gaps=gaps), t))
    for n in (17, 18, 54):
        for lead in (3, 13, 32):   # head's granules begin before, inside and at its first byte
            t = [(b'cmap', blob(lead, n)), (b'head', head[:n]), (b'post', blob(9, 3))]
            c.append(('head-%d-bytes-behind-%d' % (n, lead), sfnt(0x00010000, t), t))
    for k in (1, 2, 17):
        tables = [(b'T%03d' % (k - i), blob(3 * i + 1, i)) for i in range(k)]
        c.append(('%d-tables' % k, sfnt(0x74727565, tables), tables))
    return c


# ---------------------------------------------------------------- rejected fonts
def rejected_fonts():
    """[(id, sfnt)]: every one is MIB_E_INVALID_ARG before any device work.  The ids' numbers are the
    items of the rejection list (woff2_write.h)."""
    blob = wf._blob
    tables = [(b'cmap', blob(40, 1)), (b'head', blob(54, 2)), (b'post', blob(21, 3))]
    good = sfnt(0x00010000, tables)
    c = [('1-empty', b''), ('1-eleven-bytes', good[:11])]
    for tag in (b'ttcf', b'wOF2', b'wOFF'):
        c.append(('2-%s' % tag.decode(), tag + good[4:]))
    c.append(('3-no-tables', good[:4] + b'\0\0' + good[6:]))
    c.append(('3-directory-past-the-input', good[:59]))
    c.append(('3-many-tables', good[:4] + b'\xff\xff' + good[6:]))
    rec = 12 + 16 * 2   # post, the last table
    c.append(('4-length-one-more', good[:rec + 12] + struct.pack('>L', 22) + good[rec + 16:]))
    c.append(('4-offset-wraps', good[:rec + 8] + struct.pack('>LL', 0xFFFFFFF0, 0x20) + good[rec + 16:]))
    c.append(('4-truncated', good[:-1]))
    c.append(('5-tag-twice', sfnt(0x00010000, [(b'cmap', blob(40, 1)), (b'post', blob(4, 2)), (b'cmap', blob(7, 3))])))
    c.append(('5-dsig-twice', sfnt(0x00010000, [(b'DSIG', blob(40, 1)), (b'post', blob(4, 2)), (b'DSIG', blob(7, 3))])))
    # 6: seventeen records of 16 MiB that all point at the same bytes (overlap is not checked)
    n = 16 << 20
    big = bytearray(struct.pack('>LHHHH', 0x00010000, 17, 0, 0, 0))
    for i in range(17):
        big += b'B%03d' % i + struct.pack('>LLL', 0, 12 + 16 * 17, n + (1 if i == 0 else 0))
    c.append(('6-lengths-above-256-MiB', bytes(big) + bytes(n + 1)))
    c.append(('7-glyf-without-loca', sfnt(0x00010000, tables + [(b'glyf', blob(10, 5))])))
    c.append(('7-loca-without-glyf', sfnt(0x00010000, tables + [(b'loca', blob(10, 5))])))
    c.append(('8-only-dsig', sfnt(0x00010000, [(b'DSIG', blob(10, 5))])))
    return c


def glyf_needs_fonts(ttf):
    """[(id, sfnt)] from a good TrueType font: what the glyf transform rejects on the host"""
    t = wf.sfnt_tables(ttf)

    def font(**kw):
        u = dict(t)
        for k, v in kw.items():
            if v is None:
                del u[k.encode()]
            else:
                u[k.encode()] = v
        return wf.assemble(0x00010000, sorted(u.items()))

    ng = struct.unpack('>H', t[b'maxp'][4:6])[0]
    return [('head-53-bytes', font(head=t[b'head'][:53])), ('no-maxp', font(maxp=None)),
            ('maxp-5-bytes', font(maxp=t[b'maxp'][:5])),
            ('short-loca', font(loca=t[b'loca'][:4 * ng + 3])),
            ('no-glyphs', font(maxp=t[b'maxp'][:4] + b'\0\0' + t[b'maxp'][6:]))]


def malformed_glyph_font(ttf):
    """a loca entry that runs backwards: found by the transform's sizing pass on the device"""
    t = wf.sfnt_tables(ttf)
    loca = bytearray(t[b'loca'])
    loca[4:8] = struct.pack('>L', len(t[b'glyf']) + 4)   # glyph 0 ends past the table
    t[b'loca'] = bytes(loca)
    return wf.assemble(0x00010000, sorted(t.items()))
