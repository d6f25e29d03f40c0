"""CPU-side checks of the sessions that take a prepared dictionary (include/brotli_amd.h,
mib_encoder_new_dictionary / mib_decoder_new_dictionary): the symbols are exported and declared,
both refuse a NULL handle and a customDictionary beside a handle before any device is touched and
before the handle is read (this file runs without a GPU), the Python mirror refuses the three bad
`dictionary` options without loading the library's device side, and freeing NULL stays harmless."""
import ctypes
import os
import re

import pytest

import brotli_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mib_encoder_new_dictionary', 'mib_decoder_new_dictionary')


class EncOpts(ctypes.Structure):   # mib_enc_opts
    _fields_ = [('quality', ctypes.c_int), ('lgwin', ctypes.c_int), ('mode', ctypes.c_int), ('size_hint', ctypes.c_uint64),
                ('dict', ctypes.c_char_p), ('dict_len', ctypes.c_uint64), ('stream_chunk', ctypes.c_uint64)]


class DecOpts(ctypes.Structure):   # mib_dec_opts
    _fields_ = [('dict', ctypes.c_char_p), ('dict_len', ctypes.c_uint64), ('max_out', ctypes.c_int64),
                ('out_window', ctypes.c_uint64)]


def _lib():
    lib = ctypes.CDLL(brotli_amd.library_path())
    for name in SYMBOLS:
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        getattr(lib, name).restype = ctypes.c_void_p
    lib.mib_encoder_free.argtypes = [ctypes.c_void_p]
    lib.mib_encoder_free.restype = None
    lib.mib_decoder_free.argtypes = [ctypes.c_void_p]
    lib.mib_decoder_free.restype = None
    return lib


# (any non-NULL pointer: every check below fails before the handle is read)
FAKE = ctypes.c_void_p(0x1000)


def test_symbols_exported_and_declared():
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'brotli_amd.h')) as f:
        text = f.read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert re.search(r'mib_encoder\s*\*\s*mib_encoder_new_dictionary\s*\(\s*const\s+mib_enc_opts\s*\*\s*\w+\s*,\s*const\s+mib_dictionary\s*\*\s*\w+\s*\)', src)
    assert re.search(r'mib_decoder\s*\*\s*mib_decoder_new_dictionary\s*\(\s*const\s+mib_dec_opts\s*\*\s*\w+\s*,\s*const\s+mib_dictionary\s*\*\s*\w+\s*\)', src)
    # the option structures keep their layout: the handle is an argument, not a field
    fields = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mib_enc_opts\s*;', src).group(1)
    assert re.findall(r'(\w+)\s*;', fields) == ['quality', 'lgwin', 'mode', 'size_hint', 'dict', 'dict_len', 'stream_chunk']
    fields = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mib_dec_opts\s*;', src).group(1)
    assert re.findall(r'(\w+)\s*;', fields) == ['dict', 'dict_len', 'max_out', 'out_window']
    # the header no longer says that sessions take no handle
    flat = re.sub(r'[\s*]+', ' ', text)
    assert 'sessions, the mib_ctx_' not in flat and 'Sessions (BrotliEncoder / BrotliDecoder' in flat


def test_null_handle_is_refused():
    lib = _lib()
    assert lib.mib_encoder_new_dictionary(None, None) is None
    assert lib.mib_decoder_new_dictionary(None, None) is None
    eo = EncOpts(9, 22, 0, 0, None, 0, 0)
    do = DecOpts(None, 0, -1, 0)
    assert lib.mib_encoder_new_dictionary(ctypes.byref(eo), None) is None
    assert lib.mib_decoder_new_dictionary(ctypes.byref(do), None) is None


def test_custom_dictionary_beside_a_handle_is_refused():
    lib = _lib()
    eo = EncOpts(9, 22, 0, 0, b'abcd', 4, 0)
    do = DecOpts(b'abcd', 4, -1, 0)
    assert lib.mib_encoder_new_dictionary(ctypes.byref(eo), FAKE) is None
    assert lib.mib_decoder_new_dictionary(ctypes.byref(do), FAKE) is None
    # (an empty customDictionary is still one: the decoder attaches it)
    do = DecOpts(b'', 0, -1, 0)
    assert lib.mib_decoder_new_dictionary(ctypes.byref(do), FAKE) is None


def test_freeing_null_stays_harmless():
    lib = _lib()
    lib.mib_encoder_free(None)
    lib.mib_decoder_free(None)


def _closed():
    """a Dictionary that was closed, made without a device"""
    d = brotli_amd.Dictionary.__new__(brotli_amd.Dictionary)
    d._h, d._n = None, 4
    return d


@pytest.mark.parametrize('cls', [brotli_amd.BrotliEncoder, brotli_amd.BrotliDecoder])
def test_python_mirror_rejects_without_a_device(cls):
    with pytest.raises(TypeError):
        cls({'dictionary': b'bytes are no handle'})
    with pytest.raises(TypeError):
        cls({'dictionary': object()})
    closed = _closed()
    assert closed.closed
    with pytest.raises(ValueError):
        cls({'dictionary': closed})
    # both kinds of dictionary at once
    with pytest.raises(ValueError):
        cls({'dictionary': closed, 'customDictionary': b'abcd'})
