"""CPU-side checks of the batched WOFF2 file decoder's C ABI (include/brotli_amd.h,
mib_woff2_decode_batch): the symbols are exported and declared, malformed calls are refused, an
empty batch touches nothing, and a batch made only of files whose container does not parse is
answered per slot without a device; mib_woff2_decode and mib_debug_sfnt_assemble, which are the
batch forms with one file and one font, keep their own argument contract (this file runs without
a GPU)."""
import ctypes
import os
import re

import _oracle
import _woff2_file as wf
import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mib_woff2_decode_batch', 'mib_force_woff2_group_bytes', 'mib_debug_sfnt_assemble_batch')


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_woff2_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_force_woff2_group_bytes.argtypes = [ctypes.c_uint64]
    lib.mib_force_woff2_group_bytes.restype = None
    lib.mib_debug_sfnt_assemble_batch.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    return lib


def _unparsable():
    """the rejection list's items 1-11: what woff2file::parse itself refuses"""
    cases = [c for c in wf.rejected_files(_oracle.decode) if not c[3] and int(c[0].split('-')[0]) <= 11]
    assert sorted({int(c[0].split('-')[0]) for c in cases}) == list(range(1, 12))
    return cases


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name


def test_empty_batch_touches_nothing():
    lib = _lib()
    assert lib.mib_woff2_decode_batch(None, 0, None, None) == 0
    outs, st = (Buf * 2)(Buf(0xdead, 99), Buf(0xdead, 99)), (ctypes.c_int * 2)(55, 55)
    assert lib.mib_woff2_decode_batch(None, 0, outs, st) == 0
    assert [(o.data, o.size) for o in outs] == [(0xdead, 99)] * 2 and list(st) == [55, 55]
    assert lib.mib_debug_sfnt_assemble_batch(None, None, None, None, None, 0, None) == 0
    lib.mib_force_woff2_group_bytes(1)
    lib.mib_force_woff2_group_bytes(0)


def test_invalid_calls():
    lib = _lib()
    k = 3
    one = ctypes.create_string_buffer(b'w', 1)

    def fresh():
        return (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))
    good = (Span * k)(Span(ctypes.addressof(one), 1), Span(None, 0), Span(None, 0))
    outs, st = fresh()
    assert lib.mib_woff2_decode_batch(None, k, outs, st) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k   # a non-zero return leaves no data
    outs, st = fresh()
    assert lib.mib_woff2_decode_batch(good, k, None, st) == wf.MIB_E_INVALID_ARG
    assert lib.mib_woff2_decode_batch(good, k, outs, None) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k
    # NULL data with a size, behind a slot that would parse no better: refused before anything else
    outs, st = fresh()
    holed = (Span * k)(Span(ctypes.addressof(one), 1), Span(None, 4), Span(None, 0))
    assert lib.mib_woff2_decode_batch(holed, k, outs, st) == wf.MIB_E_INVALID_ARG
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k and list(st) == [55] * k
    # the assembly diagnostic: NULL arrays with k > 0
    assert lib.mib_debug_sfnt_assemble_batch(None, None, None, None, None, 1, outs) == wf.MIB_E_INVALID_ARG


def test_batch_of_unparsable_files_needs_no_device():
    lib = _lib()
    cases = _unparsable()
    k = len(cases)
    keep = [ctypes.create_string_buffer(c[1], max(len(c[1]), 1)) for c in cases]
    spans = (Span * k)(*[Span(ctypes.addressof(b) if len(c[1]) else None, len(c[1])) for b, c in zip(keep, cases)])
    outs, st = (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))
    assert lib.mib_woff2_decode_batch(spans, k, outs, st) == 0
    assert list(st) == [wf.MIB_E_INVALID_ARG] * k, [c[0] for c, s in zip(cases, st) if s != wf.MIB_E_INVALID_ARG]
    assert [(o.data, o.size) for o in outs] == [(None, 0)] * k


def test_solo_decode_argument_contract_needs_no_device():
    """mib_woff2_decode is the batch with k = 1: its own argument checks, and a file that does not
    parse is refused before the device is touched"""
    lib = _lib()
    lib.mib_woff2_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    one = ctypes.create_string_buffer(b'wOF2', 4)
    assert lib.mib_woff2_decode(ctypes.addressof(one), 4, None) == wf.MIB_E_INVALID_ARG
    out = Buf(0xdead, 99)
    assert lib.mib_woff2_decode(None, 4, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)
    for name, file, _, _ in _unparsable():
        keep = ctypes.create_string_buffer(file, max(len(file), 1))
        out = Buf(0xdead, 99)
        assert lib.mib_woff2_decode(ctypes.addressof(keep) if len(file) else None, len(file), ctypes.byref(out)) == \
            wf.MIB_E_INVALID_ARG, name
        assert (out.data, out.size) == (None, 0), name


def test_solo_assemble_argument_contract():
    """mib_debug_sfnt_assemble is the batch with one font, but its k counts tables: none is an error"""
    lib = _lib()
    lib.mib_debug_sfnt_assemble.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p]
    tag = (ctypes.c_uint32 * 1)(0x636D6170)
    byte = ctypes.create_string_buffer(b'x', 1)
    table = (Span * 1)(Span(ctypes.addressof(byte), 1))
    out = Buf(0xdead, 99)
    assert lib.mib_debug_sfnt_assemble(0x00010000, tag, table, None, 0, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)
    out = Buf(0xdead, 99)
    assert lib.mib_debug_sfnt_assemble(0x00010000, None, table, None, 1, ctypes.byref(out)) == wf.MIB_E_INVALID_ARG
    assert (out.data, out.size) == (None, 0)


def test_python_mirror_surface():
    assert 'woff2_decode_batch' in brotli_amd.__all__
    assert brotli_amd.woff2_decode_batch([]) == []
    assert brotli_amd.debug_sfnt_assemble_batch([]) == []
    cases = _unparsable()
    out = brotli_amd.woff2_decode_batch([c[1] for c in cases] + [bytearray(b'wOF2')])
    assert len(out) == len(cases) + 1
    assert all(isinstance(e, brotli_amd.BrotliError) and e.code == wf.MIB_E_INVALID_ARG for e in out)
    brotli_amd.force_woff2_group_bytes(1)
    brotli_amd.force_woff2_group_bytes(0)
