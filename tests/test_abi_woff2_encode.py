"""CPU-side checks of the WOFF2 writer's C ABI (include/brotli_amd.h, mib_woff2_encode and
mib_woff2_encode_batch): the symbols are exported and declared, malformed calls are refused and
leave their outputs zeroed, an empty batch touches nothing, and a batch made only of fonts the
host plan rejects is answered per slot without a device (this file runs without a GPU)."""
import ctypes
import os
import re

import _woff2_file as wf
import _woff2_write as ww
import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mib_woff2_encode', 'mib_woff2_encode_batch')


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Opts(ctypes.Structure):
    _fields_ = [('quality', ctypes.c_int), ('lgwin', ctypes.c_int), ('transforms', ctypes.c_uint32)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_woff2_encode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_woff2_encode_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name
    assert re.search(r'#define\s+MIB_WOFF2_GLYF\s+1u', src) and re.search(r'#define\s+MIB_WOFF2_HMTX\s+2u', src)
    assert 'mib_woff2_enc_opts' in src


def test_empty_batch_touches_nothing():
    lib = _lib()
    assert lib.mib_woff2_encode_batch(None, 0, None, None, None) == 0
    outs, st = (Buf * 2)(Buf(0xdead, 99), Buf(0xdead, 99)), (ctypes.c_int * 2)(55, 55)
    assert lib.mib_woff2_encode_batch(None, 0, None, outs, st) == 0
    assert [(o.data, o.size) for o in outs] == [(0xdead, 99)] * 2 and list(st) == [55, 55]


def test_invalid_calls():
    lib = _lib()
    k = 3
    one = ctypes.create_string_buffer(b'w', 1)

    def fresh():
        return (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))
    good = (Span * k)(Span(ctypes.addressof(one), 1), Span(None, 0), Span(None, 0))
    outs, st = fresh()
    assert lib.mib_woff2_encode_batch(None, k, None, outs, st) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k   # a non-zero return leaves no data
    outs, st = fresh()
    assert lib.mib_woff2_encode_batch(good, k, None, None, st) == wf.MIB_E_INVALID_ARG
    assert lib.mib_woff2_encode_batch(good, k, None, outs, None) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k
    # NULL data with a size, behind a slot that would parse no better: refused before anything else
    outs, st = fresh()
    holed = (Span * k)(Span(ctypes.addressof(one), 1), Span(None, 4), Span(None, 0))
    assert lib.mib_woff2_encode_batch(holed, k, None, outs, st) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k and list(st) == [55] * k
    # unknown transforms bits: the call's own answer, whatever the fonts are
    outs, st = fresh()
    for bits in (4, 0x80000000, 7):
        o = Opts(11, 22, bits)
        assert lib.mib_woff2_encode_batch(good, k, ctypes.byref(o), outs, st) == wf.MIB_E_INVALID_ARG, bits
        assert [(b.data, b.size) for b in outs] == [(None, 0)] * k
    # the solo call
    assert lib.mib_woff2_encode(ctypes.addressof(one), 1, None, None) == wf.MIB_E_INVALID_ARG
    out = Buf(0xdead, 99)
    assert lib.mib_woff2_encode(None, 4, None, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)
    out = Buf(0xdead, 99)
    assert lib.mib_woff2_encode(None, 0, None, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG   # fewer than 12 bytes
    assert (out.data, out.size) == (None, 0)
    out = Buf(0xdead, 99)
    o = Opts(11, 22, 8)
    assert lib.mib_woff2_encode(ctypes.addressof(one), 1, ctypes.byref(o), ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)


def test_batch_of_rejected_fonts_needs_no_device():
    lib = _lib()
    cases = ww.rejected_fonts()
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(1, 9))
    k = len(cases)
    keep = [ctypes.create_string_buffer(c[1], max(len(c[1]), 1)) for c in cases]
    spans = (Span * k)(*[Span(ctypes.addressof(b) if len(c[1]) else None, len(c[1])) for b, c in zip(keep, cases)])
    for o in (None, Opts(5, 18, 0), Opts(99, -3, 3)):
        outs, st = (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))
        assert lib.mib_woff2_encode_batch(spans, k, ctypes.byref(o) if o else None, outs, st) == 0
        assert list(st) == [wf.MIB_E_INVALID_ARG] * k, [c[0] for c, s in zip(cases, st) if s != wf.MIB_E_INVALID_ARG]
        assert [(b.data, b.size) for b in outs] == [(None, 0)] * k
    out = Buf(0xdead, 99)
    assert lib.mib_woff2_encode(ctypes.addressof(keep[2]), len(cases[2][1]), None, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)


def test_python_mirror_surface():
    assert 'woff2_encode' in brotli_amd.__all__ and 'woff2_encode_batch' in brotli_amd.__all__
    assert brotli_amd.woff2_encode_batch([]) == []
    cases = ww.rejected_fonts()
    out = brotli_amd.woff2_encode_batch([c[1] for c in cases] + [bytearray(b'true')], {'quality': 5, 'transformHmtx': False})
    assert len(out) == len(cases) + 1
    assert all(isinstance(e, brotli_amd.BrotliError) and e.code == wf.MIB_E_INVALID_ARG for e in out)
    try:
        brotli_amd.woff2_encode(cases[3][1])
        assert False, 'accepted'
    except brotli_amd.BrotliError as e:
        assert e.code == wf.MIB_E_INVALID_ARG
