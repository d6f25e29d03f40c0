"""CPU-side checks of the WOFF2 writer's C ABI over collections (include/brotli_amd.h,
mib_woff2_encode / mib_woff2_encode_batch with an OpenType collection in a slot, and the
diagnostic mib_debug_tables_equal): the collections that the host plan rejects (items 10 - 20 of
woff2_write_ttc.h's list) are answered per slot without a device, in solo and batch calls, beside
single fonts that are rejected too (this file runs without a GPU)."""
import ctypes
import os
import re

import _woff2_collection_write as cw
import _woff2_file as wf
import _woff2_write as ww
import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    lib.mib_debug_tables_equal.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_void_p]
    return lib


def _cases():
    c = cw.rejected_collections() + [('20-' + name, ttc) for name, ttc in cw.glyf_needs_collections()]
    assert sorted({int(name.split('-')[0]) for name, _ in c}) == list(range(10, 21))
    return c


def test_symbol_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        text = f.read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert hasattr(lib, 'mib_debug_tables_equal') and re.search(r'\bmib_debug_tables_equal\s*\(', src)
    # the documents no longer say that the writer rejects collections
    assert 'a first tag of ttcf' not in text
    for doc in ('DESIGN.md', 'README.md'):
        with open(os.path.join(ROOT, doc)) as f:
            assert 'writer still rejects' not in f.read(), doc


def test_debug_tables_equal_refuses_malformed_calls_without_a_device():
    lib = _lib()
    assert lib.mib_debug_tables_equal(None, None, None, None, 0, None) == 0
    one = ctypes.create_string_buffer(b'ab', 2)
    a, b = (Span * 1)(Span(ctypes.addressof(one), 2)), (Span * 1)(Span(ctypes.addressof(one), 1))
    differ = (ctypes.c_uint8 * 1)(9)
    assert lib.mib_debug_tables_equal(a, b, None, None, 1, differ) == wf.MIB_E_INVALID_ARG   # two sizes
    assert lib.mib_debug_tables_equal(a, a, None, None, 1, None) == wf.MIB_E_INVALID_ARG
    assert lib.mib_debug_tables_equal(None, a, None, None, 1, differ) == wf.MIB_E_INVALID_ARG
    mis = (ctypes.c_uint8 * 1)(16)
    assert lib.mib_debug_tables_equal(a, a, mis, None, 1, differ) == wf.MIB_E_INVALID_ARG
    assert differ[0] == 9


def test_rejected_collections_need_no_device():
    lib = _lib()
    cases = _cases() + ww.rejected_fonts()[:3]
    k = len(cases)
    keep = [ctypes.create_string_buffer(c[1], max(len(c[1]), 1)) for c in cases]
    spans = (Span * k)(*[Span(ctypes.addressof(b) if len(c[1]) else None, len(c[1])) for b, c in zip(keep, cases)])
    for o in (None, Opts(5, 18, 3), Opts(99, -3, 1)):
        outs, st = (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))
        assert lib.mib_woff2_encode_batch(spans, k, ctypes.byref(o) if o else None, outs, st) == 0
        assert list(st) == [wf.MIB_E_INVALID_ARG] * k, [c[0] for c, s in zip(cases, st) if s != wf.MIB_E_INVALID_ARG]
        assert [(b.data, b.size) for b in outs] == [(None, 0)] * k
    for i, (name, ttc) in enumerate(cases):
        out = Buf(0xdead, 99)
        assert lib.mib_woff2_encode(ctypes.addressof(keep[i]) if len(ttc) else None, len(ttc), None,
                                    ctypes.byref(out)) == wf.MIB_E_INVALID_ARG, name
        assert (out.data, out.size) == (None, 0), name
    # items 10 - 19 do not depend on the transforms
    upto19 = [i for i, c in enumerate(cases) if c[0].split('-')[0].isdigit() and 10 <= int(c[0].split('-')[0]) <= 19]
    o = Opts(5, 18, 0)
    for i in upto19:
        out = Buf(0xdead, 99)
        assert lib.mib_woff2_encode(ctypes.addressof(keep[i]), len(cases[i][1]), ctypes.byref(o), ctypes.byref(out)) == \
            wf.MIB_E_INVALID_ARG, cases[i][0]


def test_python_mirror():
    cases = _cases()
    out = brotli_amd.woff2_encode_batch([c[1] for c in cases[:12]], {'quality': 5})
    assert all(isinstance(e, brotli_amd.BrotliError) and e.code == wf.MIB_E_INVALID_ARG for e in out)
    assert brotli_amd.debug_tables_equal([]) == []
