"""Goldens for the inverse WOFF2 transforms (woff2_reconstruct_glyf / woff2_reconstruct_hmtx):
what fontTools makes of a transformed glyf table -- WOFF2GlyfTable.reconstruct, compile with
padding 4 and recalcBBoxes off, WOFF2LocaTable.compile -- for the two TrueType bench fonts
(sizes and sha256) and for a small synthetic font in full, once with each indexToLocFormat.
The synthetic font's glyphs are the edge cases of the formats (synthetic_glyphs below).
Nothing is written unless fontTools' own transform of each reconstructed table gives the
transformed table back, and its hmtx reconstruction gives the font's hmtx back.  Run on the
CPU:
    python3 tests/golden/woff2/make_reconstruct_golden.py"""
import base64
import hashlib
import io
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

OUT = os.path.join(HERE, 'reconstruct_golden.json')
INSTR_LENGTHS = (0, 1, 252, 253, 505, 762, 4000)
CONTOUR_POINTS = (252, 253, 505, 506, 761, 762)


def _bytecode(n, salt):
    return bytes((salt + 7 * i) & 0xFF for i in range(n))


def _draw(pen, pts, off=()):
    """One closed contour through pts; indices in `off` are off-curve points."""
    pen.moveTo(pts[0])
    i = 1
    while i < len(pts):
        if i in off:
            j = i
            while j in off:
                j += 1
            pen.qCurveTo(*(pts[i:j] + [pts[j] if j < len(pts) else pts[0]]))
            i = j + 1
        else:
            pen.lineTo(pts[i])
            i += 1
    pen.closePath()


def _walk(deltas, start=(0, 0)):
    x, y = start
    pts = []
    for dx, dy in deltas:
        x, y = x + dx, y + dy
        pts.append((x, y))
    return pts


def _zigzag(n, step=3):
    """n points, every delta after the first in the one-byte triplet classes"""
    pts = [(10, 10)]
    for i in range(1, n):
        x, y = pts[-1]
        pts.append((x + step, y) if i % 2 else (x, y + (step if (i // 2) % 2 else -step + 1)))
    return pts


def synthetic_glyphs():
    """(name, glyph) in glyph order, and the edits made after the pen (instructions, an
    explicit box, the overlap flag)."""
    from fontTools.pens.ttGlyphPen import TTGlyphPen
    glyphs, edits = [], {}

    def simple(name, contours, off=()):
        pen = TTGlyphPen(None)
        for pts in contours:
            _draw(pen, pts, off)
        glyphs.append((name, pen.glyph()))

    glyphs.append(('.notdef', TTGlyphPen(None).glyph()))   # the empty glyph
    simple('box', [[(0, 0), (0, 500), (400, 500), (400, 0)]])
    # every triplet class, both signs: x = 0, y = 0 (below and above 1280), < 65, < 769, < 4096, >= 4096
    d = [(0, 100), (0, -37), (0, 1279), (0, -1279), (0, 1280), (0, -2000), (120, 0), (-7, 0), (1279, 0), (-1279, 0),
         (1300, 0), (-1281, 0), (1, 1), (64, -64), (-33, 17), (-64, 64), (65, 1), (-768, 768), (300, -700), (768, 2),
         (769, 1), (-4095, 4095), (2000, -3000), (-1, 4095), (4096, 1), (-5000, 6000), (12000, -4096), (-4097, -9000),
         (255, -255), (256, -256), (-255, 255), (-256, 256), (3, 0), (0, 3)]
    simple('classes', [_walk(d, (5, 5))], off=(3, 4, 9, 20))
    # more than 258 points of one flag and one delta: the repeat count's cap at 255 (and a second run)
    simple('run600', [_walk([(5, 3)] * 600, (0, 0))])
    # 255UInt16 forms of the point counts
    for n in CONTOUR_POINTS:
        simple('pts%d' % n, [_zigzag(n)])
    simple('multi', [_zigzag(253), [(0, 0), (50, 0), (50, 50)], _zigzag(12, 5)])
    # instruction lengths
    for n in INSTR_LENGTHS:
        name = 'instr%d' % n
        simple(name, [[(0, 0), (100, 0), (100, 100 + n % 50), (0, 100)]])
        edits[name] = {'program': _bytecode(n, n)}
    simple('bboxed', [[(10, 10), (200, 10), (200, 300)]])
    edits['bboxed'] = {'bbox': (10, 10, 207, 333)}   # not its points' bounds
    simple('overlap', [[(0, 0), (300, 0), (300, 300), (0, 300)], [(100, 100), (400, 100), (400, 400)]])
    edits['overlap'] = {'overlap': True}

    def composite(name, comps):
        pen = TTGlyphPen(dict(glyphs))
        for base, t in comps:
            pen.addComponent(base, t)
        glyphs.append((name, pen.glyph()))

    composite('c_bytes', [('box', (1, 0, 0, 1, 10, -20)), ('bboxed', (1, 0, 0, 1, -128, 127))])
    composite('c_words', [('box', (1, 0, 0, 1, 300, -129)), ('box', (1, 0, 0, 1, 128, 0))])
    composite('c_scale', [('box', (0.5, 0, 0, 0.5, 0, 0))])
    composite('c_xy', [('box', (0.5, 0, 0, 0.75, 20, 30)), ('overlap', (1, 0, 0, 1, 0, 0))])
    composite('c_2x2', [('box', (0.5, 0.25, -0.25, 0.5, 1000, 7)), ('box', (-1.5, 0, 0, 1.25, 0, 0))])
    composite('c_instr', [('box', (1, 0, 0, 1, 5, 5)), ('instr1', (1, 0, 0, 1, 400, 0))])
    edits['c_instr'] = {'program': _bytecode(300, 99)}
    composite('c_instr0', [('box', (1, 0, 0, 1, 0, 9))])
    edits['c_instr0'] = {'program': b''}   # WE_HAVE_INSTRUCTIONS with a length of 0
    # monospaced tail: equal advances, so that numberOfHMetrics < numGlyphs
    for i in range(3):
        simple('mono%d' % i, [[(20 + i, 0), (300, 0), (300, 300 + i)]])
    return glyphs, edits


def synthetic_font():
    """The synthetic TrueType font's bytes (indexToLocFormat 0)."""
    from fontTools.fontBuilder import FontBuilder
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables import ttProgram
    glyphs, edits = synthetic_glyphs()
    order = [n for n, _ in glyphs]
    fb = FontBuilder(1000, isTTF=True)
    fb.setupGlyphOrder(order)
    fb.setupCharacterMap({0x41 + i: n for i, n in enumerate(order[1:])})
    fb.setupGlyf(dict(glyphs))
    glyf = fb.font['glyf']
    for name, e in edits.items():
        g = glyf[name]
        if 'program' in e:
            g.program = ttProgram.Program()
            g.program.fromBytecode(e['program'])
        if 'bbox' in e:
            g.xMin, g.yMin, g.xMax, g.yMax = e['bbox']
        if e.get('overlap'):
            g.flags[0] |= 0x40
    metrics = {}
    for i, n in enumerate(order):
        adv = 600 if n.startswith('mono') else 500 + 10 * i
        metrics[n] = (adv, getattr(glyf[n], 'xMin', 0))
    fb.setupHorizontalMetrics(metrics)
    fb.setupHorizontalHeader(ascent=800, descent=-200)
    fb.setupNameTable({'familyName': 'Reconstruct', 'styleName': 'Regular'})
    fb.setupOS2()
    fb.setupPost()
    fb.font.recalcBBoxes = False
    fb.font.recalcTimestamp = False
    buf = io.BytesIO()
    fb.font.save(buf)
    ttf = buf.getvalue()
    # the font as read back has what was asked for
    f = TTFont(io.BytesIO(ttf))
    g = f['glyf']
    assert f['head'].indexToLocFormat == 0
    assert g['.notdef'].numberOfContours == 0
    for n in CONTOUR_POINTS:
        assert g['pts%d' % n].endPtsOfContours == [n - 1], n
    assert g['run600'].endPtsOfContours == [599]
    for n in INSTR_LENGTHS:
        assert len(g['instr%d' % n].program.getBytecode()) == n
    assert len(g['c_instr'].program.getBytecode()) == 300 and g['c_instr'].isComposite()
    assert g['overlap'].flags[0] & 0x40
    assert f['hhea'].numberOfHMetrics < len(order)
    return ttf


def transform_as(ttf, index_format):
    """fontTools' transformed glyf of the font, with the header's indexFormat forced"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.woff2 import WOFF2GlyfTable
    font = TTFont(io.BytesIO(ttf))
    glyf = font['glyf']   # (read with the font's own loca format)
    font['head'].indexToLocFormat = index_format
    t = WOFF2GlyfTable()
    t.__dict__.update(glyf.__dict__)
    return t.transform(font)


def reconstruct(ttf, tglyf):
    """(glyf, loca, font holding the reconstructed tables): the procedure the GPU code matches"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.woff2 import WOFF2GlyfTable, WOFF2LocaTable
    font = TTFont(io.BytesIO(ttf))
    font.recalcBBoxes = False
    for tag in ('head', 'maxp', 'hhea'):
        font[tag]
    g = WOFF2GlyfTable()
    g.reconstruct(tglyf, font)
    g.padding = 4
    loca = WOFF2LocaTable()
    font['loca'] = loca
    font['glyf'] = g
    glyf_bytes = g.compile(font)
    loca_bytes = loca.compile(font)
    return glyf_bytes, loca_bytes, font


def spliced(ttf, glyf, loca, index_format):
    """the font with these glyf / loca bytes in place of its own"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables.DefaultTable import DefaultTable
    font = TTFont(io.BytesIO(ttf))
    font.recalcBBoxes = False
    font.recalcTimestamp = False
    for tag, data in (('glyf', glyf), ('loca', loca)):
        t = DefaultTable(tag)
        t.data = data
        font[tag] = t
    font['head'].indexToLocFormat = index_format
    buf = io.BytesIO()
    font.save(buf)
    return buf.getvalue()


def checked_reconstruct(ttf, tglyf):
    """reconstruct(), refusing a table that fontTools does not transform back to tglyf"""
    fmt = struct.unpack('>H', tglyf[6:8])[0]
    glyf, loca, font = reconstruct(ttf, tglyf)
    again = make_golden.transform(spliced(ttf, glyf, loca, fmt))
    assert again == tglyf, 'fontTools transform(reconstruct(T)) != T'
    return glyf, loca, font


def hmtx_of(ttf):
    off, length = make_golden._table(ttf, b'hmtx')
    return ttf[off:off + length]


def checked_hmtx(ttf, font, thmtx):
    """the font's hmtx, refusing it unless fontTools reconstructs it from thmtx"""
    from fontTools.ttLib.woff2 import WOFF2HmtxTable
    h = WOFF2HmtxTable()
    h.reconstruct(thmtx, font)
    want = hmtx_of(ttf)
    assert h.compile(font) == want, 'fontTools hmtx reconstruct + compile != the font\'s hmtx'
    return want


def generate():
    out = {'generator': 'fontTools WOFF2GlyfTable.reconstruct + compile (padding 4, recalcBBoxes off), '
                        'WOFF2LocaTable.compile', 'bench': {}, 'synthetic': {}}
    for name, ttf in make_golden.fonts():
        tglyf = make_golden.transform(ttf)
        glyf, loca, _ = checked_reconstruct(ttf, tglyf)
        out['bench'][name] = {'tglyf_sha256': hashlib.sha256(tglyf).hexdigest(),
                              'glyf_size': len(glyf), 'glyf_sha256': hashlib.sha256(glyf).hexdigest(),
                              'loca_size': len(loca), 'loca_sha256': hashlib.sha256(loca).hexdigest()}
    base = synthetic_font()
    variants = dict(make_golden.hmtx_variants(base))
    for fmt, tag in ((0, 'asis'), (1, 'prop')):
        ttf = variants[tag]
        tglyf = transform_as(ttf, fmt)
        glyf, loca, font = checked_reconstruct(ttf, tglyf)
        thmtx = make_golden.transform_hmtx(ttf)
        assert thmtx is not None
        hmtx = checked_hmtx(ttf, font, thmtx)
        b64 = lambda b: base64.b64encode(b).decode()   # noqa: E731
        out['synthetic']['fmt%d' % fmt] = {
            'tglyf': b64(tglyf), 'glyf': b64(glyf), 'loca': b64(loca), 'hmtx': b64(hmtx), 'thmtx': b64(thmtx),
            'num_glyphs': struct.unpack('>H', tglyf[4:6])[0], 'num_hmetrics': font['hhea'].numberOfHMetrics}
    return out


def main():
    out = generate()
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for k, v in out['bench'].items():
        print(k, v)
    for k, v in out['synthetic'].items():
        print(k, {a: (len(base64.b64decode(b)) if isinstance(b, str) else b) for a, b in v.items()})


if __name__ == '__main__':
    main()
