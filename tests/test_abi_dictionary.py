"""CPU-side checks of the prepared dictionary's C ABI (include/brotli_amd.h, mib_dictionary_* and
the two batch calls that take one): the symbols are exported and declared, every documented
MIB_E_INVALID_ARG comes back before any device is touched (this file runs without a GPU), k == 0
returns 0, and NULL handles are harmless to free and to size."""
import ctypes
import os
import re

import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB_E_INVALID_ARG = -101
SYMBOLS = ('mib_dictionary_new', 'mib_dictionary_free', 'mib_dictionary_size', 'mib_encode_batch_dictionary',
           'mib_decode_batch_dictionary')


class Opts(ctypes.Structure):   # mib_enc_opts
    _fields_ = [('quality', ctypes.c_int), ('lgwin', ctypes.c_int), ('mode', ctypes.c_int), ('size_hint', ctypes.c_uint64),
                ('dict', ctypes.c_char_p), ('dict_len', ctypes.c_uint64), ('stream_chunk', ctypes.c_uint64)]


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_char_p), ('size', ctypes.c_size_t)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_dictionary_new.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.mib_dictionary_free.argtypes = [ctypes.c_void_p]
    lib.mib_dictionary_free.restype = None
    lib.mib_dictionary_size.argtypes = [ctypes.c_void_p]
    lib.mib_dictionary_size.restype = ctypes.c_uint64
    lib.mib_encode_batch_dictionary.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decode_batch_dictionary.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p]
    return lib


# (any non-NULL pointer: every check below fails before the handle is read)
FAKE = ctypes.c_void_p(0x1000)


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name
    assert re.search(r'typedef\s+struct\s+mib_dictionary\s+mib_dictionary\s*;', src)
    # the span follows from the record's 24-bit distance field, per lgwin
    m = re.search(r'#define\s+MIB_DICTIONARY_MATCH_SPAN\(lgwin\)\s+(.*)', src)
    assert m and eval(m.group(1).replace('u', '').replace('lgwin', '22')) == 0xFFFFFE - ((1 << 22) - 16)
    # the option structures keep their layout
    fields = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mib_enc_opts\s*;', src).group(1)
    assert re.findall(r'(\w+)\s*;', fields) == ['quality', 'lgwin', 'mode', 'size_hint', 'dict', 'dict_len', 'stream_chunk']
    fields = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mib_dec_opts\s*;', src).group(1)
    assert re.findall(r'(\w+)\s*;', fields) == ['dict', 'dict_len', 'max_out', 'out_window']


def test_dictionary_new_rejects_before_any_device_work():
    lib = _lib()
    assert lib.mib_dictionary_new(b'abcd', 4, None) == MIB_E_INVALID_ARG
    h = ctypes.c_void_p(0xdead)
    assert lib.mib_dictionary_new(None, 4, ctypes.byref(h)) == MIB_E_INVALID_ARG and h.value is None
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        h = ctypes.c_void_p(0xdead)
        assert lib.mib_dictionary_new(b'abcd', n, ctypes.byref(h)) == MIB_E_INVALID_ARG and h.value is None


def test_null_handles_are_harmless():
    lib = _lib()
    lib.mib_dictionary_free(None)
    assert lib.mib_dictionary_size(None) == 0


def test_batch_calls_reject_before_any_device_work():
    lib = _lib()
    spans = (Span * 1)(Span(b'abc', 3))
    outs, st = (Buf * 1)(), (ctypes.c_int * 1)()
    # a NULL handle, with and without streams
    assert lib.mib_encode_batch_dictionary(spans, 1, None, None, outs, st) == MIB_E_INVALID_ARG
    assert lib.mib_decode_batch_dictionary(spans, 1, None, -1, outs, st) == MIB_E_INVALID_ARG
    assert lib.mib_encode_batch_dictionary(None, 0, None, None, None, None) == MIB_E_INVALID_ARG
    assert lib.mib_decode_batch_dictionary(None, 0, None, -1, None, None) == MIB_E_INVALID_ARG
    # o->dict together with a handle
    o = Opts(11, 22, 0, 0, b'abcd', 4, 0)
    assert lib.mib_encode_batch_dictionary(spans, 1, ctypes.byref(o), FAKE, outs, st) == MIB_E_INVALID_ARG
    assert lib.mib_encode_batch_dictionary(None, 0, ctypes.byref(o), FAKE, None, None) == MIB_E_INVALID_ARG
    # NULL arrays with k > 0, NULL data with a size
    for args in ((None, outs, st), (spans, None, st), (spans, outs, None)):
        assert lib.mib_encode_batch_dictionary(args[0], 1, None, FAKE, args[1], args[2]) == MIB_E_INVALID_ARG
        assert lib.mib_decode_batch_dictionary(args[0], 1, FAKE, -1, args[1], args[2]) == MIB_E_INVALID_ARG
    hole = (Span * 1)(Span(None, 3))
    assert lib.mib_encode_batch_dictionary(hole, 1, None, FAKE, outs, st) == MIB_E_INVALID_ARG
    assert lib.mib_decode_batch_dictionary(hole, 1, FAKE, -1, outs, st) == MIB_E_INVALID_ARG
    assert lib.mib_decode_batch_dictionary(spans, 1, FAKE, -2, outs, st) == MIB_E_INVALID_ARG
    assert outs[0].data is None and outs[0].size == 0


def test_empty_batches_need_no_device():
    lib = _lib()
    assert lib.mib_encode_batch_dictionary(None, 0, None, FAKE, None, None) == 0
    assert lib.mib_decode_batch_dictionary(None, 0, FAKE, -1, None, None) == 0


def test_python_mirror_rejects_without_a_device():
    import pytest
    with pytest.raises(TypeError):
        brotli_amd.encode_batch([b'abc'], dictionary=b'bytes are no handle')
    with pytest.raises(TypeError):
        brotli_amd.decode_batch([b'abc'], dictionary=object())
    with pytest.raises(ValueError):
        brotli_amd.decode_batch([b'abc'], options={'maxOutputSize': 5})
