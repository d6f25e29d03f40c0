"""CPU-side checks of the collection decoder's C ABI (include/brotli_amd.h): the diagnostic
mib_debug_ttc_assemble is exported and declared and refuses what is no collection before it
touches a device, and collections whose container does not parse (items 14 - 20 of the rejection
list) are answered without a device, alone and as a batch (this file runs without a GPU)."""
import ctypes
import os
import re

import _woff2_collection as wc
import _woff2_file as wf
import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_debug_ttc_assemble.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.mib_woff2_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def test_symbol_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert hasattr(lib, 'mib_debug_ttc_assemble')
    assert re.search(r'\bmib_debug_ttc_assemble\s*\(', src)
    assert 'debug_ttc_assemble' in dir(brotli_amd)


def test_diagnostic_argument_contract_needs_no_device():
    lib = _lib()
    tags = (ctypes.c_uint32 * 2)(0x636D6170, 0x6E616D65)
    byte = ctypes.create_string_buffer(b'xy', 2)
    tables = (Span * 2)(Span(ctypes.addressof(byte), 1), Span(ctypes.addressof(byte) + 1, 1))
    flavors, counts, idx = (ctypes.c_uint32 * 1)(wc.V1), (ctypes.c_uint32 * 1)(2), (ctypes.c_uint32 * 2)(0, 1)

    def call(version=wc.V1, tags=tags, tables=tables, k=2, flavors=flavors, counts=counts, idx=idx, nf=1):
        out = Buf(0xdead, 99)
        rc = lib.mib_debug_ttc_assemble(version, tags, tables, None, k, flavors, counts, idx, nf, ctypes.byref(out))
        assert (out.data, out.size) == (None, 0)
        return rc

    assert lib.mib_debug_ttc_assemble(wc.V1, tags, tables, None, 2, flavors, counts, idx, 1, None) == wf.MIB_E_INVALID_ARG
    for kw in (dict(tags=None), dict(tables=None), dict(flavors=None), dict(counts=None), dict(idx=None), dict(k=0), dict(nf=0),
               dict(version=0), dict(version=0x00030000), dict(nf=65536), dict(k=65536),
               dict(counts=(ctypes.c_uint32 * 1)(0)), dict(idx=(ctypes.c_uint32 * 2)(0, 2)), dict(idx=(ctypes.c_uint32 * 2)(1, 1))):
        assert call(**kw) == wf.MIB_E_INVALID_ARG, sorted(kw)


def test_unparsable_collections_need_no_device():
    lib = _lib()
    cases = wc.rejected_collections()
    for name, file, _ in cases:
        keep = ctypes.create_string_buffer(file, len(file))
        out = Buf(0xdead, 99)
        assert lib.mib_woff2_decode(ctypes.addressof(keep), len(file), ctypes.byref(out)) == wf.MIB_E_INVALID_ARG, name
        assert (out.data, out.size) == (None, 0), name
    out = brotli_amd.woff2_decode_batch([c[1] for c in cases])
    assert all(isinstance(e, brotli_amd.BrotliError) and e.code == wf.MIB_E_INVALID_ARG for e in out)
