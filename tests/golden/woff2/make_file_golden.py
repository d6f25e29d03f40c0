"""Goldens for woff2_decode: real .woff2 files and the sfnt each stands for.

The files are written by fontTools' own WOFF2 writer (flavor 'woff2', recalcBBoxes and
recalcTimestamp off), once with its default transforms (glyf, loca) and once with hmtx
transformed as well, from the synthetic font of make_reconstruct_golden.synthetic_font(), the
two TrueType bench fonts and (one variant: nothing to transform) the CFF bench font.  fontTools
needs a `brotli` module for that; inside this script only, the module is a small object around
the repository's oracle (tests/_oracle.py), whose quality is recorded in the JSON.

The expected sfnt follows the layout rules of brotli-lib_amd/csrc/woff2_file.h, stated in
Python by tests/_woff2_file.assemble: untransformed tables are their bytes of the
oracle-decoded stream, cut by the file's directory; glyf and loca are what
make_reconstruct_golden.reconstruct compiles (padding 4, boxes kept -- NOT what
WOFF2Reader['glyf'] gives, which pads with fontTools' default); hmtx is
WOFF2HmtxTable.reconstruct + compile.  Nothing is written unless fontTools accepts each sfnt
with its checksums verified, loads it, reads every table but glyf, loca and head out of the
.woff2 as the same bytes, and transforms the expected glyf back into the file's.

The synthetic files and sfnts are stored in full (file_golden.json), the bench fonts' .woff2
files beside it, their sfnts as size and sha256.  Run on the CPU:
    python3 tests/golden/woff2/make_file_golden.py"""
import base64
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts tests/ on the path)
import make_reconstruct_golden as rec  # noqa: E402
import _oracle  # noqa: E402
import _woff2_file as wf  # noqa: E402

OUT = os.path.join(HERE, 'file_golden.json')
ORACLE_QUALITY = 11
VARIANTS = (('', ('glyf', 'loca')), ('-hmtx', ('glyf', 'loca', 'hmtx')))


class _OracleBrotli:
    """what fontTools.ttLib.woff2 uses of the brotli module"""
    MODE_GENERIC, MODE_TEXT, MODE_FONT = 0, 1, 2

    @staticmethod
    def compress(data, mode=0, **kw):
        return _oracle.encode(bytes(data), ORACLE_QUALITY, 22, mode)

    @staticmethod
    def decompress(data):
        return _oracle.decode(bytes(data))


def _fonttools():
    import fontTools.ttLib.woff2 as w2
    w2.brotli = _OracleBrotli
    w2.haveBrotli = True
    return w2


def _fixed_dates(sfnt):
    """the font with head's created / modified set to a constant (FontBuilder stamps the time
    of the run, and head is part of these goldens)"""
    from fontTools.ttLib import TTFont
    font = TTFont(io.BytesIO(sfnt), recalcBBoxes=False, recalcTimestamp=False)
    font['head'].created = font['head'].modified = 3800000000   # seconds since 1904: mid-2024
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def sources():
    """(name, sfnt bytes, variants)"""
    yield 'synthetic', _fixed_dates(rec.synthetic_font()), VARIANTS
    for name, ttf in make_golden.fonts():
        yield name, ttf, VARIANTS
    with open(os.path.join(make_golden.TESTS, 'golden', 'bench', 'enc-otf.bin'), 'rb') as f:
        yield 'enc-otf', f.read(), VARIANTS[:1]


def write_woff2(sfnt, transformed):
    from fontTools.ttLib import TTFont
    w2 = _fonttools()
    font = TTFont(io.BytesIO(sfnt), recalcBBoxes=False, recalcTimestamp=False)
    font.flavor = 'woff2'
    font.flavorData = w2.WOFF2FlavorData(transformedTables=transformed)
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def expected_sfnt(sfnt, woff2):
    """the sfnt the file stands for, refused unless fontTools agrees with it (see above)"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.sfnt import SFNTReader
    w2 = _fonttools()
    flavor, entries, comp = wf.parse(woff2)
    tables = wf.cut(entries, _oracle.decode(comp))
    state = {e[0]: wf.is_transformed(e[0], e[1]) for e in entries}
    tglyf = None
    if state.get(b'glyf'):
        assert state[b'loca'] and tables[b'loca'] == b''
        tglyf = tables[b'glyf']
        glyf, loca, font = rec.reconstruct(sfnt, tglyf)
        tables[b'glyf'], tables[b'loca'] = glyf, loca
        if state.get(b'hmtx'):
            h = w2.WOFF2HmtxTable()
            h.reconstruct(tables[b'hmtx'], font)
            tables[b'hmtx'] = h.compile(font)
    else:
        assert not state.get(b'hmtx')
    out = wf.assemble(flavor, [(e[0], tables[e[0]]) for e in entries])
    SFNTReader(io.BytesIO(out), checkChecksums=2)   # raises on a table or file checksum that is off
    TTFont(io.BytesIO(out))
    theirs = w2.WOFF2Reader(io.BytesIO(woff2))
    for tag, data in tables.items():
        if tag not in (b'glyf', b'loca', b'head'):
            assert theirs[tag.decode('latin-1')] == data, tag
    if tglyf is not None:
        assert make_golden.transform(out) == tglyf, 'fontTools transform(expected glyf) != the file\'s'
    return out


def generate():
    """(the JSON's content, {file name: bytes} of the binary fixtures)"""
    import fontTools
    out = {'generator': 'fontTools %s WOFF2 writer (flavor woff2, recalcBBoxes / recalcTimestamp off) over the '
                        'repository\'s oracle as its brotli module' % fontTools.version,
           'oracle_quality': ORACLE_QUALITY, 'synthetic': {}, 'bench': {}}
    files = {}
    b64 = lambda b: base64.b64encode(b).decode()   # noqa: E731
    for name, sfnt, variants in sources():
        for suffix, transformed in variants:
            woff2 = write_woff2(sfnt, transformed)
            want = expected_sfnt(sfnt, woff2)
            fx = {'woff2_size': len(woff2), 'woff2_sha256': hashlib.sha256(woff2).hexdigest(),
                  'sfnt_size': len(want), 'sfnt_sha256': hashlib.sha256(want).hexdigest()}
            if name == 'synthetic':
                fx['woff2'], fx['sfnt'] = b64(woff2), b64(want)
                out['synthetic'][name + suffix] = fx
            else:
                fx['file'] = name + suffix + '.woff2'
                files[fx['file']] = woff2
                out['bench'][name + suffix] = fx
    return out, files


def main():
    out, files = generate()
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for name, data in files.items():
        with open(os.path.join(HERE, name), 'wb') as f:
            f.write(data)
    for group in ('synthetic', 'bench'):
        for k, v in out[group].items():
            print(k, {a: b for a, b in v.items() if a not in ('woff2', 'sfnt')})


if __name__ == '__main__':
    main()
