"""CPU-side checks of the streaming decoder's C ABI (include/brotli_amd.h, mib_decoder_*): the
symbols are exported and declared, the option defaults are the documented ones, and NULL
arguments are refused before any device is touched (this file runs without a GPU)."""
import ctypes
import os
import re

import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB_E_INVALID_ARG = -101
SYMBOLS = ('mib_dec_opts_default', 'mib_decoder_new', 'mib_decoder_update', 'mib_decoder_finish',
           'mib_decoder_is_finished', 'mib_decoder_free')


class DecOpts(ctypes.Structure):
    _fields_ = [('dict', ctypes.c_void_p), ('dict_len', ctypes.c_uint64), ('max_out', ctypes.c_int64),
                ('out_window', ctypes.c_uint64)]


class Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    lib.mib_decoder_new.restype = ctypes.c_void_p
    lib.mib_decoder_new.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.mib_decoder_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mib_decoder_is_finished.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_free.argtypes = [ctypes.c_void_p]
    lib.mib_dec_opts_default.argtypes = [ctypes.c_void_p]
    return lib


def _header():
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)


def test_symbols_exported_and_declared():
    lib, src = _lib(), _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r'\b%s\s*\(' % name, src), name
    assert re.search(r'typedef\s+struct\s+mib_decoder\s+mib_decoder\s*;', src)
    fields = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mib_dec_opts\s*;', src).group(1)
    assert re.findall(r'(\w+)\s*;', fields) == ['dict', 'dict_len', 'max_out', 'out_window']


def test_opts_default():
    o = DecOpts(0xdead, 77, 5, 9)
    _lib().mib_dec_opts_default(ctypes.byref(o))
    assert (o.dict, o.dict_len, o.max_out, o.out_window) == (None, 0, -1, 0)
    _lib().mib_dec_opts_default(None)   # tolerated


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib()
    out = Buf(0xdead, 99)
    one = ctypes.create_string_buffer(b'\x06', 1)
    assert lib.mib_decoder_update(None, one, 1, ctypes.byref(out)) == MIB_E_INVALID_ARG
    assert lib.mib_decoder_finish(None, ctypes.byref(out)) == MIB_E_INVALID_ARG
    assert lib.mib_decoder_is_finished(None) == 0
    lib.mib_decoder_free(None)
    d = lib.mib_decoder_new(None)   # NULL options: the defaults
    assert d
    try:
        assert lib.mib_decoder_update(d, one, 1, None) == MIB_E_INVALID_ARG
        assert lib.mib_decoder_update(d, None, 1, ctypes.byref(out)) == MIB_E_INVALID_ARG
        assert lib.mib_decoder_finish(d, None) == MIB_E_INVALID_ARG
        assert lib.mib_decoder_is_finished(d) == 0
        # an empty update decodes nothing and needs no device
        out = Buf(0xdead, 99)
        assert lib.mib_decoder_update(d, None, 0, ctypes.byref(out)) == 0
        assert out.size == 0
        lib.mib_buf_free(ctypes.byref(out))
    finally:
        lib.mib_decoder_free(d)
    # a dictionary length without a dictionary, a limit below "none"
    assert not lib.mib_decoder_new(ctypes.byref(DecOpts(None, 5, -1, 0)))
    assert not lib.mib_decoder_new(ctypes.byref(DecOpts(None, 0, -2, 0)))


def test_python_mirror_surface():
    assert 'BrotliDecoder' in brotli_amd.__all__
    d = brotli_amd.BrotliDecoder({'outWindow': 65536, 'maxOutputSize': 10, 'customDictionary': b'abc'})
    assert d.finished is False
    assert d.update(b'') == b''
    for name in ('update', 'finish'):
        assert callable(getattr(d, name))
