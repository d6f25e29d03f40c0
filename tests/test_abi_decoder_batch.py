"""CPU-side checks of the batched streaming decoder's C ABI (include/brotli_amd.h,
mib_decoder_update_batch / mib_decoder_finish_batch): the symbols are exported and declared,
malformed calls are refused before any session is touched, and a batch of empty chunks needs
no device (this file runs without a GPU)."""
import ctypes
import os
import re

import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB_E_INVALID_ARG = -101
SYMBOLS = ('mib_decoder_update_batch', 'mib_decoder_finish_batch', 'mib_decoder_batch_stats', 'mib_force_decoder_grid')


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_decoder_new.restype = ctypes.c_void_p
    lib.mib_decoder_new.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_free.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_is_finished.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_stats.restype = None
    lib.mib_decoder_update_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_finish_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_batch_stats.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_batch_stats.restype = None
    lib.mib_force_decoder_grid.argtypes = [ctypes.c_int]
    lib.mib_force_decoder_grid.restype = None
    lib.mib_buf_free.argtypes = [ctypes.c_void_p]
    return lib


def _passes(lib, d):
    p = ctypes.c_uint64(77)
    lib.mib_decoder_stats(d, ctypes.byref(p), None)
    return p.value


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name


def test_empty_batch_and_null_stats():
    lib = _lib()
    assert lib.mib_decoder_update_batch(None, None, 0, None, None) == 0
    assert lib.mib_decoder_finish_batch(None, 0, None, None) == 0
    lib.mib_decoder_batch_stats(None)   # tolerated
    n, m = ctypes.c_uint64(5), ctypes.c_uint64(7)
    lib.mib_decoder_batch_stats(ctypes.byref(n))
    assert lib.mib_decoder_update_batch(None, None, 0, None, None) == 0
    lib.mib_decoder_batch_stats(ctypes.byref(m))
    assert n.value == m.value   # an empty call launches nothing
    lib.mib_force_decoder_grid(3)
    lib.mib_force_decoder_grid(0)


def test_invalid_calls_change_no_session():
    lib = _lib()
    k = 3
    hs = (ctypes.c_void_p * k)(*[lib.mib_decoder_new(None) for _ in range(k)])
    assert all(hs)
    one = ctypes.create_string_buffer(b'\x06', 1)
    try:
        def fresh():
            return (Buf * k)(*[Buf(0xdead, 99) for _ in range(k)]), (ctypes.c_int * k)(*([55] * k))

        def spans(*items):
            return (Span * k)(*[Span(p, n) for p, n in items])
        good = spans((ctypes.addressof(one), 1), (None, 0), (None, 0))
        bad_calls = []
        outs, st = fresh()
        # NULL arrays with k > 0
        bad_calls.append(lib.mib_decoder_update_batch(None, good, k, outs, st))
        bad_calls.append(lib.mib_decoder_update_batch(hs, None, k, outs, st))
        bad_calls.append(lib.mib_decoder_update_batch(hs, good, k, None, st))
        bad_calls.append(lib.mib_decoder_update_batch(hs, good, k, outs, None))
        bad_calls.append(lib.mib_decoder_finish_batch(None, k, outs, st))
        bad_calls.append(lib.mib_decoder_finish_batch(hs, k, None, st))
        bad_calls.append(lib.mib_decoder_finish_batch(hs, k, outs, None))
        # a NULL handle (behind a valid one with data)
        holed = (ctypes.c_void_p * k)(hs[0], None, hs[2])
        bad_calls.append(lib.mib_decoder_update_batch(holed, good, k, outs, st))
        bad_calls.append(lib.mib_decoder_finish_batch(holed, k, outs, st))
        # NULL data with a size
        bad_calls.append(lib.mib_decoder_update_batch(hs, spans((ctypes.addressof(one), 1), (None, 4), (None, 0)), k, outs, st))
        # the same handle twice
        twice = (ctypes.c_void_p * k)(hs[0], hs[1], hs[0])
        bad_calls.append(lib.mib_decoder_update_batch(twice, good, k, outs, st))
        bad_calls.append(lib.mib_decoder_finish_batch(twice, k, outs, st))
        assert bad_calls == [MIB_E_INVALID_ARG] * len(bad_calls)
        # nothing was touched: results and statuses as they were, no session opened or failed
        assert [(o.data, o.size) for o in outs] == [(0xdead, 99)] * k and list(st) == [55] * k
        for h in hs:
            assert _passes(lib, h) == 0 and lib.mib_decoder_is_finished(h) == 0
        # ... and each session still takes an empty update: 0 and empty, with no device
        outs, st = fresh()
        assert lib.mib_decoder_update_batch(hs, spans((None, 0), (ctypes.addressof(one), 0), (None, 0)), k, outs, st) == 0
        assert list(st) == [0] * k and [o.size for o in outs] == [0] * k
        for o in outs:
            lib.mib_buf_free(ctypes.byref(o))
    finally:
        for h in hs:
            lib.mib_decoder_free(h)


def test_python_mirror_surface():
    assert 'decoder_update_batch' in brotli_amd.__all__ and 'decoder_finish_batch' in brotli_amd.__all__
    ds = [brotli_amd.BrotliDecoder({'outWindow': 65536}) for _ in range(3)]
    assert brotli_amd.decoder_update_batch(ds, [b'', bytearray(), b'']) == [b'', b'', b'']
    assert brotli_amd.decoder_update_batch([], []) == []
    assert brotli_amd.decoder_finish_batch([]) == []
    assert [d.finished for d in ds] == [False] * 3
