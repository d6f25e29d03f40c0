"""CPU-side checks of the device-resident session calls' C ABI (include/brotli_amd.h,
mib_decoder_update_batch_device / mib_decoder_finish_batch_device / mib_decoder_held_output /
mib_debug_copy_batch): the symbols are exported and declared, malformed calls are refused before
any session is touched, and a batch of empty chunks on fresh sessions needs no device (this file
runs without a GPU; no device pointer is ever dereferenced here)."""
import ctypes
import os
import re

import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB_E_INVALID_ARG = -101
SYMBOLS = ('mib_decoder_update_batch_device', 'mib_decoder_finish_batch_device', 'mib_decoder_held_output',
           'mib_debug_copy_batch')
FAKE = 0x7000000000   # stands for a device address: a refused or empty call never reads it


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    lib.mib_decoder_new.restype = ctypes.c_void_p
    lib.mib_decoder_new.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_free.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_is_finished.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_stats.restype = None
    lib.mib_decoder_update_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_finish_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_held_output.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_held_output.restype = ctypes.c_uint64
    lib.mib_debug_copy_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def _passes(lib, d):
    p = ctypes.c_uint64(77)
    lib.mib_decoder_stats(d, ctypes.byref(p), None)
    return p.value


def _u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        text = f.read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name
    assert re.search(r'#define\s+MIB_DEC_MORE_OUTPUT\s+1\b', src)
    assert brotli_amd.MORE_OUTPUT == 1


def test_empty_batch_and_null_handle():
    lib = _lib()
    assert lib.mib_decoder_update_batch_device(None, None, None, 0, None, None, None, None) == 0
    assert lib.mib_decoder_finish_batch_device(None, 0, None, None, None, None) == 0
    assert lib.mib_decoder_held_output(None) == 0
    assert lib.mib_debug_copy_batch(None, None, None, 0) == 0
    assert lib.mib_debug_copy_batch(None, None, None, 2) == MIB_E_INVALID_ARG


def test_invalid_calls_change_no_session():
    lib = _lib()
    k = 3
    hs = (ctypes.c_void_p * k)(*[lib.mib_decoder_new(None) for _ in range(k)])
    assert all(hs)
    try:
        def fresh():
            return _u64(*([99] * k)), (ctypes.c_int * k)(*([55] * k))
        ioff, ooff = _u64(0, 1, 1, 5), _u64(0, 10, 10, 27)
        sizes, st = fresh()
        upd, fin = lib.mib_decoder_update_batch_device, lib.mib_decoder_finish_batch_device
        bad = []
        # NULL arrays with k > 0
        bad.append(upd(None, FAKE, ioff, k, FAKE, ooff, sizes, st))
        bad.append(upd(hs, FAKE, None, k, FAKE, ooff, sizes, st))
        bad.append(upd(hs, FAKE, ioff, k, FAKE, None, sizes, st))
        bad.append(upd(hs, FAKE, ioff, k, FAKE, ooff, None, st))
        bad.append(upd(hs, FAKE, ioff, k, FAKE, ooff, sizes, None))
        bad.append(fin(None, k, FAKE, ooff, sizes, st))
        bad.append(fin(hs, k, FAKE, None, sizes, st))
        bad.append(fin(hs, k, FAKE, ooff, None, st))
        bad.append(fin(hs, k, FAKE, ooff, sizes, None))
        # NULL buffers whose offsets span bytes
        bad.append(upd(hs, None, ioff, k, FAKE, ooff, sizes, st))
        bad.append(upd(hs, FAKE, ioff, k, None, ooff, sizes, st))
        bad.append(fin(hs, k, None, ooff, sizes, st))
        # a NULL handle (behind a valid one with data)
        holed = (ctypes.c_void_p * k)(hs[0], None, hs[2])
        bad.append(upd(holed, FAKE, ioff, k, FAKE, ooff, sizes, st))
        bad.append(fin(holed, k, FAKE, ooff, sizes, st))
        # the same handle twice
        twice = (ctypes.c_void_p * k)(hs[0], hs[1], hs[0])
        bad.append(upd(twice, FAKE, ioff, k, FAKE, ooff, sizes, st))
        bad.append(fin(twice, k, FAKE, ooff, sizes, st))
        # decreasing offsets, input and output, behind a slot with data
        bad.append(upd(hs, FAKE, _u64(0, 4, 3, 5), k, FAKE, ooff, sizes, st))
        bad.append(upd(hs, FAKE, ioff, k, FAKE, _u64(0, 10, 9, 27), sizes, st))
        bad.append(fin(hs, k, FAKE, _u64(5, 10, 20, 19), sizes, st))
        assert bad == [MIB_E_INVALID_ARG] * len(bad)
        # nothing was touched: sizes and statuses as they were, no session opened, failed or holding
        assert list(sizes) == [99] * k and list(st) == [55] * k
        for h in hs:
            assert _passes(lib, h) == 0 and lib.mib_decoder_is_finished(h) == 0 and lib.mib_decoder_held_output(h) == 0
    finally:
        for h in hs:
            lib.mib_decoder_free(h)


def test_all_empty_chunks_need_no_device():
    """fresh sessions, empty chunks (at odd offsets), rooms of 0 and more: 0 everywhere, no launch"""
    lib = _lib()
    k = 3
    hs = (ctypes.c_void_p * k)(*[lib.mib_decoder_new(None) for _ in range(k)])
    try:
        sizes, st = _u64(*([99] * k)), (ctypes.c_int * k)(*([55] * k))
        assert lib.mib_decoder_update_batch_device(hs, FAKE, _u64(3, 3, 3, 3), k, FAKE, _u64(1, 1, 18, 4096), sizes, st) == 0
        assert list(sizes) == [0] * k and list(st) == [0] * k
        # ... with no buffers at all
        sizes, st = _u64(*([99] * k)), (ctypes.c_int * k)(*([55] * k))
        assert lib.mib_decoder_update_batch_device(hs, None, _u64(0, 0, 0, 0), k, None, _u64(0, 0, 0, 0), sizes, st) == 0
        assert list(sizes) == [0] * k and list(st) == [0] * k
        for h in hs:
            assert _passes(lib, h) == 0 and lib.mib_decoder_is_finished(h) == 0 and lib.mib_decoder_held_output(h) == 0
    finally:
        for h in hs:
            lib.mib_decoder_free(h)


def test_python_mirror_surface():
    for name in ('decoder_update_batch_device', 'decoder_finish_batch_device', 'MORE_OUTPUT'):
        assert name in brotli_amd.__all__ and hasattr(brotli_amd, name), name
    ds = [brotli_amd.BrotliDecoder({'outWindow': 65536}) for _ in range(3)]
    assert brotli_amd.decoder_update_batch_device(ds, FAKE, [7, 7, 7, 7], FAKE, [0, 5, 5, 9]) == ([0, 0, 0], [0, 0, 0])
    assert brotli_amd.decoder_update_batch_device([], None, [0], None, [0]) == ([], [])
    assert brotli_amd.decoder_finish_batch_device([], None, [0]) == ([], [])
    assert [d.held_output for d in ds] == [0, 0, 0] and [d.finished for d in ds] == [False] * 3
    try:
        brotli_amd.decoder_update_batch_device(ds, FAKE, [0, 0, 0], FAKE, [0, 0, 0, 0])
        raise AssertionError('a short offset list was accepted')
    except ValueError:
        pass
    try:   # call-level errors raise
        brotli_amd.decoder_update_batch_device(ds, FAKE, [0, 2, 1, 3], FAKE, [0, 0, 0, 0])
        raise AssertionError('decreasing offsets were accepted')
    except brotli_amd.BrotliError as e:
        assert e.code == MIB_E_INVALID_ARG
