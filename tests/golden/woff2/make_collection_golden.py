"""Goldens for woff2_decode of font collections: .woff2 files of flavor ttcf and the TTC each
stands for (DESIGN.md 4c "A font collection").

fontTools does not write (or read) WOFF2 collections, so the container is written here
(tests/_woff2_collection.write_collection) around fontTools' own transforms: the members are
datagen.glyf_font fonts with the metrics of _woff2_file.font_with_metrics (deterministic), their
transformed glyf and hmtx are WOFF2GlyfTable / WOFF2HmtxTable.transform's, and the stream is
compressed by the repository's oracle.  The expected TTC follows the layout rules stated in
Python by _woff2_collection.assemble_collection; its reconstructed tables are taken the way
make_file_golden.expected_sfnt takes them (make_reconstruct_golden.reconstruct: padding 4, boxes
kept; WOFF2HmtxTable.reconstruct + compile).  Nothing is written unless fontTools opens every
member of every TTC with its checksums verified.

  ttc-shared-glyf  version 1.0: two fonts share one transformed glyf / loca pair, a transformed
                   hmtx, hhea, head and maxp; each has a name table of its own
  ttc-two-glyf     version 2.0: two fonts (flavors 0x00010000 and 'true') with their own
                   transformed pairs, the first with a transformed hmtx, the second with a plain
                   one; the second lists its tables in another order than the directory's; one
                   directory entry is listed by no font
  ttc-null         version 1.0: one font, glyf and loca with the null transform

Run on the CPU:
    python3 tests/golden/woff2/make_collection_golden.py"""
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
import make_file_golden  # noqa: E402
import _oracle  # noqa: E402
import _woff2_collection as wc  # noqa: E402
import _woff2_file as wf  # noqa: E402

sys.path.insert(0, os.path.join(make_golden.TESTS, '..', 'brotli-lib_amd', 'python'))

OUT = os.path.join(HERE, 'collection_golden.json')
ORACLE_QUALITY = 11
MODE_FONT = 2


def member(seed, nglyphs):
    """a six-table TrueType font: head, hhea, hmtx, maxp, glyf, loca"""
    from brotli_amd import datagen
    return wf.font_with_metrics(datagen.glyf_font(seed, nglyphs))


def _name(text):
    """a name table of one Macintosh record"""
    import struct
    s = text.encode('ascii')
    return struct.pack('>HHH', 0, 1, 18) + struct.pack('>HHHHHH', 1, 0, 0, 4, len(s), 0) + s


class _Font:
    """a member's tables, as the stream holds them and as the TTC is to hold them"""

    def __init__(self, ttf, glyf_transformed=True, hmtx_transformed=True):
        w2 = make_file_golden._fonttools()
        self.ttf = ttf
        self.plain = wf.sfnt_tables(ttf)
        self.want = dict(self.plain)
        self.stream = dict(self.plain)
        self.version = {}
        if glyf_transformed:
            tglyf = make_golden.transform(ttf)
            glyf, loca, font = rec.reconstruct(ttf, tglyf)
            self.stream[b'glyf'], self.stream[b'loca'] = tglyf, b''
            self.want[b'glyf'], self.want[b'loca'] = glyf, loca
            if hmtx_transformed:
                thmtx = make_golden.transform_hmtx(ttf)
                assert thmtx is not None
                h = w2.WOFF2HmtxTable()
                h.reconstruct(thmtx, font)
                self.stream[b'hmtx'], self.want[b'hmtx'] = thmtx, h.compile(font)
                self.version[b'hmtx'] = 1
        else:
            assert not hmtx_transformed
            self.version[b'glyf'] = self.version[b'loca'] = 3

    def entry(self, tag):
        """(the directory entry, the stream's bytes, the TTC's bytes)"""
        v = self.version.get(tag, 0)
        s = self.stream[tag]
        tlen = len(s) if wf.is_transformed(tag, v) else None
        return [tag, v, len(self.plain[tag]), tlen], s, self.want[tag]


def _extra(tag, data):
    return [tag, 0, len(data), None], data, data


def build(version, rows, fonts):
    """(.woff2 bytes, TTC bytes) of rows = [(entry, stream bytes, TTC bytes)]"""
    entries = [r[0] for r in rows]
    stream = b''.join(r[1] for r in rows)
    woff2 = wc.write_collection(version, entries, fonts, _oracle.encode(stream, ORACLE_QUALITY, 22, MODE_FONT))
    ttc = wc.assemble_collection(version, [(r[0][0], r[2]) for r in rows], fonts)
    return woff2, ttc


def files():
    """{name: (.woff2 bytes, TTC bytes)}"""
    a, b = _Font(member(101, 120)), _Font(member(202, 90), hmtx_transformed=False)
    out = {}
    order = (b'head', b'hhea', b'hmtx', b'maxp', b'glyf', b'loca')
    rows = [a.entry(t) for t in order] + [_extra(b'name', _name('Collection One')), _extra(b'name', _name('Collection Two, Bold'))]
    out['ttc-shared-glyf'] = build(wc.V1, rows, [(wc.V1, [0, 1, 2, 3, 4, 5, 6]), (wc.V1, [0, 1, 2, 3, 4, 5, 7])])
    rows = [a.entry(t) for t in order] + [_extra(b'DSIG', bytes(range(23)))] + [b.entry(t) for t in order]
    out['ttc-two-glyf'] = build(wc.V2, rows, [(wc.V1, [0, 1, 2, 3, 4, 5]), (wc.TRUE, [12, 11, 10, 9, 8, 7])])
    c = _Font(member(303, 40), glyf_transformed=False, hmtx_transformed=False)
    rows = [c.entry(t) for t in (b'glyf', b'loca', b'head', b'hhea', b'hmtx', b'maxp')]
    out['ttc-null'] = build(wc.V1, rows, [(wc.V1, [0, 1, 2, 3, 4, 5])])
    return out


def check(woff2, ttc):
    """fontTools opens every member with its checksums verified and finds the listed tables"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.sfnt import SFNTReader
    _, entries, fonts, _ = wc.parse_collection(woff2)
    for m, (flavor, idx) in enumerate(fonts):
        r = SFNTReader(io.BytesIO(ttc), checkChecksums=2, fontNumber=m)
        assert sorted(r.keys()) == sorted(entries[i][0].decode('latin-1') for i in idx)
        TTFont(io.BytesIO(ttc), fontNumber=m)['glyf']


def generate():
    import fontTools
    out = {'generator': 'tests/_woff2_collection.write_collection around fontTools %s WOFF2GlyfTable / WOFF2HmtxTable.transform, '
                        'the stream compressed by the repository\'s oracle' % fontTools.version,
           'oracle_quality': ORACLE_QUALITY, 'files': {}}
    b64 = lambda b: base64.b64encode(b).decode()   # noqa: E731
    for name, (woff2, ttc) in files().items():
        check(woff2, ttc)
        out['files'][name] = {'woff2': b64(woff2), 'woff2_size': len(woff2), 'woff2_sha256': hashlib.sha256(woff2).hexdigest(),
                              'ttc': b64(ttc), 'ttc_size': len(ttc), 'ttc_sha256': hashlib.sha256(ttc).hexdigest(), 'code': 0}
    return out


def main():
    out = generate()
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for k, v in out['files'].items():
        print(k, {a: b for a, b in v.items() if a not in ('woff2', 'ttc')})


if __name__ == '__main__':
    main()
