"""Shared by the WOFF2 file tests and tests/golden/woff2/make_file_golden.py: the container in
pure Python -- directory parser and writer, the sfnt assembler that states the layout rules of
brotli-lib_amd/csrc/woff2_file.h (the expectation of both the host and the device assembly),
the fixtures of tests/golden/woff2/file_golden.json and the files that must be rejected."""
import base64
import json
import os
import struct

import _inputs

HERE = os.path.join(_inputs.GOLDEN, 'woff2')
KNOWN_TAGS = (b'cmap', b'head', b'hhea', b'hmtx', b'maxp', b'name', b'OS/2', b'post', b'cvt ', b'fpgm', b'glyf',
              b'loca', b'prep', b'CFF ', b'VORG', b'EBDT', b'EBLC', b'gasp', b'hdmx', b'kern', b'LTSH', b'PCLT',
              b'VDMX', b'vhea', b'vmtx', b'BASE', b'GDEF', b'GPOS', b'GSUB', b'EBSC', b'JSTF', b'MATH', b'CBDT',
              b'CBLC', b'COLR', b'CPAL', b'SVG ', b'sbix', b'acnt', b'avar', b'bdat', b'bloc', b'bsln', b'cvar',
              b'fdsc', b'feat', b'fmtx', b'fvar', b'gvar', b'hsty', b'just', b'lcar', b'mort', b'morx', b'opbd',
              b'prop', b'trak', b'Zapf', b'Silf', b'Glat', b'Gloc', b'Feat', b'Sill')
HEAD_MAGIC = 0xB1B0AFBA
MIB_E_INVALID_ARG = -101


# ---------------------------------------------------------------- the sfnt's layout
def checksum(data):
    data = data + b'\0' * (-len(data) % 4)
    return sum(struct.unpack('>%dL' % (len(data) // 4), data)) & 0xFFFFFFFF


def assemble(flavor, tables):
    """The sfnt of [(tag, bytes)]: records sorted by tag, table data in the list's order, each at
    a 4-byte boundary and zero-padded; head's bytes 8..11 zero in its checksum and then
    0xB1B0AFBA - the file's sum."""
    k = len(tables)
    sel = 0
    while (2 << sel) <= k:
        sel += 1
    out = bytearray(struct.pack('>LHHHH', flavor, k, ((1 << sel) * 16) & 0xFFFF, sel, (k * 16 - (1 << sel) * 16) & 0xFFFF))
    at = 12 + 16 * k
    body = bytearray()
    recs, head_at = [], None
    for tag, data in tables:
        data = bytes(data)
        if tag == b'head' and len(data) >= 12:
            data = data[:8] + bytes(4) + data[12:]
            head_at = at + len(body)
        recs.append((tag, checksum(data), at + len(body), len(data)))
        body += data + b'\0' * (-len(data) % 4)
    for tag, cs, off, length in sorted(recs):
        out += tag + struct.pack('>LLL', cs, off, length)
    out += body
    if head_at is not None:
        out[head_at + 8:head_at + 12] = struct.pack('>L', (HEAD_MAGIC - checksum(bytes(out))) & 0xFFFFFFFF)
    return bytes(out)


def sfnt_tables(sfnt):
    """{tag: bytes} of an sfnt"""
    k = struct.unpack('>H', sfnt[4:6])[0]
    out = {}
    for i in range(k):
        tag, _, off, length = struct.unpack('>4sLLL', sfnt[12 + 16 * i:28 + 16 * i])
        out[tag] = sfnt[off:off + length]
    return out


# ---------------------------------------------------------------- the container
def base128(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    return bytes(reversed(out))


def _read_base128(b, at):
    v = 0
    for i in range(5):
        c = b[at + i]
        v = (v << 7) | (c & 0x7F)
        if not c & 0x80:
            return v, at + i + 1
    raise ValueError('UIntBase128')


def is_transformed(tag, version):
    return version == 0 if tag in (b'glyf', b'loca') else (tag == b'hmtx' and version == 1)


def parse(data):
    """(flavor, [[tag, version, origLength, transformLength or None]], compressed stream) of a
    well-formed file"""
    sig, flavor, length, k, _, _, comp = struct.unpack('>4sLLHHLL', data[:24])
    assert sig == b'wOF2' and length == len(data)
    at = 48
    entries = []
    for _ in range(k):
        flags = data[at]
        at += 1
        if flags & 63 == 63:
            tag = data[at:at + 4]
            at += 4
        else:
            tag = KNOWN_TAGS[flags & 63]
        orig, at = _read_base128(data, at)
        tlen = None
        if is_transformed(tag, flags >> 6):
            tlen, at = _read_base128(data, at)
        entries.append([tag, flags >> 6, orig, tlen])
    return flavor, entries, data[at:at + comp]


def write(flavor, entries, compressed, known=True):
    """A .woff2 file.  entries: [tag, version, origLength, transformLength or None]; a length may
    be raw bytes (a malformed UIntBase128).  No metadata, no private block."""
    d = b''
    for tag, version, orig, tlen in entries:
        if known and tag in KNOWN_TAGS:
            d += bytes([KNOWN_TAGS.index(tag) | (version << 6)])
        else:
            d += bytes([63 | (version << 6)]) + tag
        d += orig if isinstance(orig, bytes) else base128(orig)
        if tlen is not None:
            d += tlen if isinstance(tlen, bytes) else base128(tlen)
    total = 48 + len(d) + len(compressed)
    head = struct.pack('>4sLLHHLLHHLLLLL', b'wOF2', flavor, total, len(entries), 0, 0, len(compressed), 1, 0, 0, 0, 0, 0, 0)
    return head + d + compressed


def stream_lengths(entries):
    """each table's length in the decompressed stream"""
    return [orig if tlen is None else tlen for _, _, orig, tlen in entries]


def cut(entries, stream):
    """{tag: its bytes in the decompressed stream}"""
    out, at = {}, 0
    for e, n in zip(entries, stream_lengths(entries)):
        out[e[0]] = stream[at:at + n]
        at += n
    assert at == len(stream)
    return out


# ---------------------------------------------------------------- fixtures
def golden():
    with open(os.path.join(HERE, 'file_golden.json')) as f:
        return json.load(f)


def golden_files():
    """[(name, .woff2 bytes, sfnt bytes or None, sfnt size, sfnt sha256)]"""
    g = golden()
    out = []
    for name, fx in sorted(g['synthetic'].items()):
        out.append((name, base64.b64decode(fx['woff2']), base64.b64decode(fx['sfnt']), fx['sfnt_size'], fx['sfnt_sha256']))
    for name, fx in sorted(g['bench'].items()):
        with open(os.path.join(HERE, fx['file']), 'rb') as f:
            out.append((name, f.read(), None, fx['sfnt_size'], fx['sfnt_sha256']))
    return out


def synthetic_file(hmtx=True):
    fx = golden()['synthetic']['synthetic-hmtx' if hmtx else 'synthetic']
    return base64.b64decode(fx['woff2'])


def _edit(entries, which, **kw):
    out = [list(e) for e in entries]
    for e in out:
        if e[0] == which:
            for k, v in kw.items():
                e[('tag', 'version', 'orig', 'tlen').index(k)] = v
    return out


def rejected_files(decompress):
    """[(id, file, stream, edited)]: every one is MIB_E_INVALID_ARG.  Made from the synthetic file
    whose hmtx is transformed; `stream` is what the file's Brotli stream decodes to, or (edited:
    the last cases) what it is to decode to once the caller has compressed it into the file
    (with_stream).  The ids' numbers are the items of the rejection list."""
    good = synthetic_file()
    flavor, ent, comp = parse(good)
    stream = decompress(comp)
    tags = [e[0] for e in ent]
    assert b'cmap' in tags and b'post' in tags and ent[tags.index(b'hmtx')][1] == 1
    cases = []

    def add(name, file, s=None):
        cases.append((name, file, s))

    def hdr(at, fmt, v):
        b = bytearray(good)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, v)
        return bytes(b)

    add('1-47-bytes', good[:47])
    add('1-empty', b'')
    add('1-signature-wOFF', b'wOFF' + good[4:])
    add('1-flavor-ttcf', hdr(4, '>4s', b'ttcf'))
    add('2-length-one-more', hdr(8, '>L', len(good) + 1))
    add('2-trailing-byte', good + b'\0')
    add('3-no-tables', hdr(12, '>H', 0))
    add('4-directory-past-the-file', hdr(8, '>L', 50)[:50])
    add('4-many-tables', hdr(12, '>H', 0xFFFF))
    add('4-compressed-size-past-the-file', hdr(20, '>L', len(good) - len(write(flavor, ent, b'')) + 1))
    n_cmap = ent[tags.index(b'cmap')][2]
    add('5-leading-0x80', write(flavor, _edit(ent, b'cmap', orig=b'\x80' + base128(n_cmap)), comp))
    add('5-six-bytes', write(flavor, _edit(ent, b'cmap', orig=b'\x81\x80\x80\x80\x80\x00'), comp))
    add('5-two-to-the-32', write(flavor, _edit(ent, b'cmap', orig=b'\x90\x80\x80\x80\x00'), comp))
    add('6-known-tag-twice', write(flavor, _edit(ent, b'post', tag=b'cmap'), comp))
    add('6-spelled-tag-twice', write(flavor, _edit(ent, b'post', tag=b'cmap'), comp, known=False))
    add('6-head-twice', write(flavor, _edit(ent, b'post', tag=b'head'), comp))
    add('7-cmap-version-1', write(flavor, _edit(ent, b'cmap', version=1), comp))
    add('7-glyf-version-1', write(flavor, _edit(ent, b'glyf', version=1), comp))
    add('7-loca-version-2', write(flavor, _edit(ent, b'loca', version=2), comp))
    add('7-hmtx-version-2', write(flavor, _edit(ent, b'hmtx', version=2), comp))
    add('7-hmtx-version-3', write(flavor, _edit(ent, b'hmtx', version=3), comp))
    add('8-loca-transform-length', write(flavor, _edit(ent, b'loca', tlen=1), comp))
    add('9-loca-null-glyf-transformed', write(flavor, _edit(ent, b'loca', version=3, orig=0, tlen=None), comp))
    add('9-glyf-without-loca', write(flavor, [e for e in ent if e[0] != b'loca'], comp))
    tglyf_n = ent[tags.index(b'glyf')][3]
    null_glyf = _edit(_edit(ent, b'glyf', version=3, orig=tglyf_n, tlen=None), b'loca', version=3, orig=0, tlen=None)
    add('10-hmtx-transformed-glyf-null', write(flavor, null_glyf, comp))
    add('10-hmtx-transformed-no-hhea', write(flavor, _edit(ent, b'hhea', tag=b'hheX'), comp))
    add('11-lengths-above-256-MiB', write(flavor, _edit(ent, b'cmap', orig=(1 << 28) + 1), comp))
    add('12-stream-one-short', write(flavor, _edit(ent, b'cmap', orig=n_cmap + 1), comp))
    add('12-stream-one-long', write(flavor, _edit(ent, b'cmap', orig=n_cmap - 1), comp))
    # 13: what the reconstruct functions reject, inside a well-formed container
    at = dict(zip(tags, _offsets(ent)))
    g0, h0 = at[b'glyf'], at[b'hmtx']
    s = bytearray(stream)
    s[g0 + 2:g0 + 4] = struct.pack('>H', 2)   # a reserved option bit of the transformed glyf
    add('13-glyf-reserved-option-bit', good, bytes(s))
    s = bytearray(stream)
    sizes = struct.unpack('>7L', stream[g0 + 8:g0 + 36])
    s[g0 + 8:g0 + 16] = struct.pack('>LL', sizes[0] - 2, sizes[1] + 2)   # the sizes still sum
    add('13-glyf-ncontour-size', good, bytes(s))
    s = bytearray(stream)
    s[h0] |= 0x04
    add('13-hmtx-reserved-bits', good, bytes(s))
    s = bytearray(stream)
    s[h0] = 0
    add('13-hmtx-neither-bit', good, bytes(s))
    return [(name, file, stream if s is None else s, s is not None) for name, file, s in cases]


def _offsets(entries):
    out, at = [], 0
    for n in stream_lengths(entries):
        out.append(at)
        at += n
    return out


def with_stream(file, stream, compress):
    """the well-formed `file` with its Brotli stream replaced by compress(stream)"""
    flavor, ent, _ = parse(file)
    return write(flavor, ent, compress(stream))


# ---------------------------------------------------------------- a file made by the product
def font_with_metrics(ttf):
    """The four-table font of datagen.glyf_font (head, maxp, loca, glyf; long loca) with an hhea
    and an hmtx whose side bearings are the glyphs' xMin, the last three glyphs monospaced."""
    t = sfnt_tables(ttf)
    ng = struct.unpack('>H', t[b'maxp'][4:6])[0]
    loca = struct.unpack('>%dL' % (ng + 1), t[b'loca'])
    xmin = [struct.unpack('>h', t[b'glyf'][loca[g] + 2:loca[g] + 4])[0] if loca[g + 1] > loca[g] else 0 for g in range(ng)]
    nhm = ng - 3
    hmtx = b''.join(struct.pack('>Hh', 400 + (7 * g) % 300, xmin[g]) for g in range(nhm))
    hmtx += b''.join(struct.pack('>h', xmin[g]) for g in range(nhm, ng))
    hhea = struct.pack('>L', 0x00010000) + bytes(30) + struct.pack('>H', nhm)
    t[b'hhea'], t[b'hmtx'] = hhea, hmtx
    return assemble(0x00010000, sorted(t.items()))


def product_file(ttf, transform_glyf, transform_hmtx, reconstruct_glyf, compress):
    """(.woff2 bytes, the sfnt it stands for) of a TrueType font, written here around the
    product's own transforms and encoder: glyf, loca and hmtx transformed, loca right behind
    glyf, the other tables in tag order.  The expectation takes glyf and loca from
    reconstruct_glyf and every other table from the font."""
    t = sfnt_tables(ttf)
    tglyf, thmtx = transform_glyf(ttf), transform_hmtx(ttf)
    assert thmtx is not None
    tags = [tag for tag in sorted(t) if tag != b'loca']
    tags.insert(tags.index(b'glyf') + 1, b'loca')
    stream, entries = b'', []
    for tag in tags:
        data = {b'glyf': tglyf, b'loca': b'', b'hmtx': thmtx}.get(tag, t[tag])
        if tag in (b'glyf', b'loca'):
            entries.append([tag, 0, len(t[tag]), len(data)])
        elif tag == b'hmtx':
            entries.append([tag, 1, len(t[tag]), len(data)])
        else:
            entries.append([tag, 0, len(data), None])
        stream += data
    flavor = struct.unpack('>L', ttf[:4])[0]
    glyf, loca = reconstruct_glyf(tglyf)
    want = dict(t)
    want[b'glyf'], want[b'loca'] = glyf, loca
    return write(flavor, entries, compress(stream)), assemble(flavor, [(tag, want[tag]) for tag in tags])


# ---------------------------------------------------------------- the assembly kernels' cases
def _blob(n, salt):
    return bytes((salt * 131 + 7 * i + (i >> 8)) & 0xFF for i in range(n))


_head = _blob   # (a head whose bytes 8..11 are not zero: the assembly has to clear them)


def assemble_cases():
    """[(id, flavor, [(tag, bytes)], misalign or None)]"""
    c = [('one-empty-table', 0x00010000, [(b'cmap', b'')], None)]
    for n in (1, 2, 3, 5, 15, 16, 17):
        c.append(('one-table-%d' % n, 0x00010000, [(b'cmap', _blob(n, n))], None))
    c.append(('small-tables-packed', 0x4F54544F, [(b'tb%02d' % n, _blob(n, n)) for n in (1, 2, 3, 5, 15, 16, 17, 0, 33)], None))
    for m in range(16):
        c.append(('misalign-%d' % m, 0x00010000, [(b'name', _blob(33, m)), (b'post', _blob(33, m + 16))], [m, (m + 5) & 15]))
    c.append(('tiles-plus-one', 0x00010000, [(b'cmap', _blob(7, 1)), (b'CFF ', _blob(3 * 4096 + 1, 2)), (b'post', _blob(9, 3))],
              [3, 1, 2]))
    c.append(('tiles-many', 0x00010000, [(b'gvar', _blob(70 * 4096 + 18, 5)), (b'head', _head(54, 6))], [0, 7]))
    # 5 words of 0xFF sum past 2^32 (4 * 0xFFFFFFFF + 0xFFFFFFFF); 4100 bytes: across a tile as well
    c.append(('sum-wraps-5-words', 0x00010000, [(b'cvt ', b'\xff' * 20)], None))
    c.append(('sum-wraps-tile', 0x00010000, [(b'cvt ', b'\xff' * 4100), (b'prep', b'\xff' * 19)], [9, 2]))
    head = _head(54, 9)
    others = [(b'cmap', _blob(40, 1)), (b'maxp', _blob(32, 2)), (b'post', _blob(21, 3))]
    c.append(('head-first', 0x00010000, [(b'head', head)] + others, None))
    c.append(('head-last', 0x00010000, others + [(b'head', head)], None))
    c.append(('head-middle-misaligned', 0x00010000, others[:1] + [(b'head', head)] + others[1:], [1, 13, 6, 15]))
    c.append(('head-alone', 0x00010000, [(b'head', head)], None))
    c.append(('head-absent', 0x00010000, others, None))
    c.append(('head-11-bytes', 0x00010000, [(b'cmap', _blob(5, 4)), (b'head', _head(11, 5))], None))
    c.append(('head-12-bytes', 0x00010000, [(b'head', _head(12, 5)), (b'cmap', _blob(5, 4))], None))
    for k in (1, 2, 3, 17):
        c.append(('%d-tables' % k, 0x74727565, [(b'T%03d' % (k - i), _blob(3 * i + 1, i)) for i in range(k)], None))
    return c
