"""Shared by the WOFF2 reconstruction tests: the fixtures of
tests/golden/woff2/reconstruct_golden.json and the fixed bad inputs that both the host build
of the walker (CPU) and the library (GPU) must reject."""
import base64
import json
import os
import struct

import _inputs

HERE = os.path.join(_inputs.GOLDEN, 'woff2')
STREAMS = ('nContour', 'nPoints', 'flag', 'glyph', 'composite', 'bbox', 'instruction')


def golden():
    with open(os.path.join(HERE, 'reconstruct_golden.json')) as f:
        return json.load(f)


def synthetic():
    """{'fmt0' | 'fmt1': fixture with its byte fields decoded}"""
    out = {}
    for name, fx in golden()['synthetic'].items():
        out[name] = {k: (base64.b64decode(v) if isinstance(v, str) else v) for k, v in fx.items()}
    return out


def stream_sizes(t):
    return list(struct.unpack('>7L', t[8:36]))


def resized(t, stream, delta, fill=b'\0'):
    """t with `stream` grown (filled) or cut at its end by delta bytes, its header size adjusted"""
    sizes = stream_sizes(t)
    i = STREAMS.index(stream)
    end = 36 + sum(sizes[:i + 1])
    body = t[:end] + fill * delta + t[end:] if delta > 0 else t[:end + delta] + t[end:]
    sizes[i] += delta
    return body[:8] + struct.pack('>7L', *sizes) + body[36:]


def first_composite(t):
    ng = struct.unpack('>H', t[4:6])[0]
    nc = struct.unpack('>%dh' % ng, t[36:36 + 2 * ng])
    return next(g for g in range(ng) if nc[g] < 0)


def bad_inputs():
    """[(id, kind, table, fixture)]: kind 'glyf' or 'hmtx'; every one is MIB_E_INVALID_ARG"""
    fx = synthetic()['fmt0']
    t, h = fx['tglyf'], fx['thmtx']
    sizes = stream_sizes(t)
    cases = [('empty', 'glyf', b''), ('35-bytes', 'glyf', t[:35]), ('trailing-byte', 'glyf', t + b'\0')]
    b = bytearray(t)   # a stream size one larger than the bytes that are there
    b[8 + 4 * 3:12 + 4 * 3] = struct.pack('>L', sizes[3] + 1)
    cases.append(('sizes-do-not-sum', 'glyf', bytes(b)))
    b = bytearray(t)   # two bytes moved from nContour to nPoints: the sum still holds
    b[8:16] = struct.pack('>LL', sizes[0] - 2, sizes[1] + 2)
    cases.append(('ncontour-size', 'glyf', bytes(b)))
    b = bytearray(t)
    b[2:4] = struct.pack('>H', 2)
    cases.append(('reserved-option-bit', 'glyf', bytes(b)))
    b = bytearray(t)
    g = first_composite(t)
    at = 36 + sum(sizes[:5]) + (g >> 3)
    assert b[at] & (0x80 >> (g & 7))
    b[at] &= ~(0x80 >> (g & 7)) & 0xFF
    cases.append(('composite-without-bbox', 'glyf', bytes(b)))
    cases.append(('npoints-one-short', 'glyf', resized(t, 'nPoints', -1)))
    cases.append(('flags-one-short', 'glyf', resized(t, 'flag', -1)))
    cases.append(('glyph-stream-one-short', 'glyf', resized(t, 'glyph', -1)))
    cases.append(('instructions-one-over', 'glyf', resized(t, 'instruction', 1)))
    cases.append(('bbox-stream-below-bitmap', 'glyf', resized(t, 'bbox', -(sizes[5] - 3))))
    cases.append(('hmtx-reserved-bits', 'hmtx', bytes([h[0] | 0x04]) + h[1:]))
    cases.append(('hmtx-neither-bit', 'hmtx', b'\0' + h[1:]))
    cases.append(('hmtx-trailing-byte', 'hmtx', h + b'\0'))
    return [(name, kind, table, fx) for name, kind, table in cases]


def with_short_loca(t):
    """t with indexFormat 0 in its header"""
    return t[:6] + b'\0\0' + t[8:]


def all_empty(ng=5):
    """(transformed glyf, glyf, loca) of a font whose glyphs are all empty: fontTools writes one
    zero byte (tests/test_woff2_reconstruct_golden.py checks that it does)"""
    bitmap = ((ng + 31) >> 5) << 2
    t = struct.pack('>HHHH7L', 0, 0, ng, 0, 2 * ng, 0, 0, 0, 0, bitmap, 0) + bytes(2 * ng) + bytes(bitmap)
    return t, b'\0', bytes(2 * (ng + 1))


def record(b):
    return struct.pack('<L', len(b)) + b
