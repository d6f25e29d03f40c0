"""Python mirror of countertype/brotli-lib's public API over the brotli_amd C ABI.

    brotliEncode(input, options)   src/encode/encode.ts:50-90
    BrotliEncoder(options)         src/encode/encode.ts:290-490
    brotliDecode(data, options)    src/decode/decode.ts:18-65   (options dict or legacy int)
    BrotliDecoder(options)         extension: the streaming decode side of BrotliEncoder
    brotliDecodedSize(data)        src/decode/decode.ts:9-11
    EncoderMode                    src/encode/enc-constants.ts:56-60

Same argument meaning and error behaviour as the reference: decoder failures raise
``BrotliError("Brotli error code: N")`` with the reference's N, ``maxOutputSize`` raises
``BrotliError("Decompressed size X exceeds limit Y")``.  All compute runs in the HIP
library (libbrotli_amd.so, built in-tree by __graft_entry__.build()); there is no CPU
fallback -- without an MI355X the calls raise.
"""
import ctypes
import os

__all__ = ['brotliEncode', 'BrotliEncoder', 'brotliDecode', 'BrotliDecoder', 'brotliDecodedSize', 'EncoderMode', 'BrotliError',
           'encode_batch', 'decode_batch', 'encoder_update_batch', 'decoder_update_batch', 'decoder_finish_batch',
           'decoder_update_batch_device', 'decoder_finish_batch_device', 'MORE_OUTPUT', 'DeviceContext', 'library_path',
           'woff2_decode', 'woff2_decode_batch', 'woff2_encode', 'woff2_encode_batch']

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# BROTLI_AMD_LIB: an instrumented build of the same library (timing experiments only)
_LIB_PATH = os.environ.get('BROTLI_AMD_LIB') or os.path.join(_PKG, 'libbrotli_amd.so')


def library_path():
    return _LIB_PATH


class EncoderMode:
    GENERIC = 0
    TEXT = 1
    FONT = 2


class BrotliError(Exception):
    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class _Opts(ctypes.Structure):
    _fields_ = [('quality', ctypes.c_int), ('lgwin', ctypes.c_int), ('mode', ctypes.c_int),
                ('size_hint', ctypes.c_uint64), ('dict', ctypes.c_char_p), ('dict_len', ctypes.c_uint64),
                ('stream_chunk', ctypes.c_uint64)]


class _DecOpts(ctypes.Structure):
    _fields_ = [('dict', ctypes.c_char_p), ('dict_len', ctypes.c_uint64), ('max_out', ctypes.c_int64),
                ('out_window', ctypes.c_uint64)]


class _Buf(ctypes.Structure):
    _fields_ = [('data', ctypes.POINTER(ctypes.c_uint8)), ('size', ctypes.c_size_t)]


class _Span(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('size', ctypes.c_size_t)]


class _Woff2EncOpts(ctypes.Structure):
    _fields_ = [('quality', ctypes.c_int), ('lgwin', ctypes.c_int), ('transforms', ctypes.c_uint32)]


class _KTime(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 32), ('ms', ctypes.c_double), ('launches', ctypes.c_uint32)]


_lib = None

# Results come back as bytes objects the library writes into (mib_set_allocator): the device
# copies its output straight into the object returned, no copy through a C buffer.
_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_FREE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
_new_bytes = ctypes.pythonapi.PyBytes_FromStringAndSize
_new_bytes.restype = ctypes.py_object
_new_bytes.argtypes = [ctypes.c_char_p, ctypes.c_ssize_t]
_results = {}   # address -> the bytes object the library is filling / has filled
_HUGE = 2 << 20
_madvise = ctypes.CDLL(None, use_errno=True).madvise
_madvise.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


def _alloc(opaque, size):
    try:
        b = _new_bytes(None, max(1, size))   # (a fresh object: b'' is a shared singleton)
    except MemoryError:
        return None
    addr = ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value
    _results[addr] = b
    if size >= _HUGE and os.environ.get('MIB_PY_HUGEPAGE') != '0':
        # large results: the copy into fresh memory is page-fault bound; 2 MiB pages fault 512x less
        lo = (addr + _HUGE - 1) & ~(_HUGE - 1)
        hi = (addr + size) & ~(_HUGE - 1)
        if hi > lo:
            _madvise(lo, hi - lo, 14)   # MADV_HUGEPAGE
    return addr


def _free(opaque, addr):
    _results.pop(addr, None)


_alloc_cb = _ALLOC_FN(_alloc)
_free_cb = _FREE_FN(_free)


def _L():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise BrotliError('brotli_amd: %s not built (run __graft_entry__.build())' % _LIB_PATH)
        # PyTorch-ROCm ships its own libamdhip64 (same soname).  Loading torch first makes the
        # library bind to that one runtime; the other order would put two HIP runtimes in the
        # process and torch's device init would fail.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(_LIB_PATH)
        u8p = ctypes.c_char_p
        lib.mib_strerror.restype = ctypes.c_char_p
        lib.mib_strerror.argtypes = [ctypes.c_int]
        lib.mib_init.argtypes = [ctypes.c_int]
        lib.mib_encode.argtypes = [u8p, ctypes.c_size_t, ctypes.POINTER(_Opts), ctypes.POINTER(_Buf)]
        lib.mib_decode.argtypes = [u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64,
                                   ctypes.POINTER(_Buf)]
        lib.mib_decoded_size.argtypes = [u8p, ctypes.c_size_t]
        lib.mib_decoded_size.restype = ctypes.c_int64
        lib.mib_buf_free.argtypes = [ctypes.POINTER(_Buf)]
        lib.mib_encoder_new.argtypes = [ctypes.POINTER(_Opts)]
        lib.mib_encoder_new.restype = ctypes.c_void_p
        lib.mib_encoder_update.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
        lib.mib_encoder_finish.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf)]
        lib.mib_encoder_free.argtypes = [ctypes.c_void_p]
        lib.mib_encoder_update_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_Span), ctypes.c_size_t,
                                                 ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_decoder_new'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_decoder_new.argtypes = [ctypes.POINTER(_DecOpts)]
            lib.mib_decoder_new.restype = ctypes.c_void_p
            lib.mib_decoder_update.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
            lib.mib_decoder_finish.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf)]
            lib.mib_decoder_is_finished.argtypes = [ctypes.c_void_p]
            lib.mib_decoder_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
            lib.mib_decoder_stats.restype = None
            lib.mib_force_decoder_build.argtypes = [ctypes.c_int]
            lib.mib_force_decoder_build.restype = None
            lib.mib_decoder_free.argtypes = [ctypes.c_void_p]
        if hasattr(lib, 'mib_decoder_update_batch'):
            lib.mib_decoder_update_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_Span), ctypes.c_size_t,
                                                     ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
            lib.mib_decoder_finish_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.POINTER(_Buf),
                                                     ctypes.POINTER(ctypes.c_int)]
            lib.mib_decoder_batch_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
            lib.mib_decoder_batch_stats.restype = None
            lib.mib_decoder_batch_times.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.mib_decoder_batch_times.restype = None
            lib.mib_force_decoder_grid.argtypes = [ctypes.c_int]
            lib.mib_force_decoder_grid.restype = None
        if hasattr(lib, 'mib_decoder_update_batch_device'):
            u64p = ctypes.POINTER(ctypes.c_uint64)
            lib.mib_decoder_update_batch_device.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, u64p, ctypes.c_size_t,
                                                            ctypes.c_void_p, u64p, u64p, ctypes.POINTER(ctypes.c_int)]
            lib.mib_decoder_finish_batch_device.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_void_p,
                                                            u64p, u64p, ctypes.POINTER(ctypes.c_int)]
            lib.mib_decoder_held_output.argtypes = [ctypes.c_void_p]
            lib.mib_decoder_held_output.restype = ctypes.c_uint64
            lib.mib_debug_copy_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), u64p,
                                                 ctypes.c_size_t]
        lib.mib_encode_batch.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Opts),
                                         ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
        lib.mib_decode_batch.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Buf),
                                         ctypes.POINTER(ctypes.c_int)]
        lib.mib_dictionary_new.argtypes = [u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        lib.mib_dictionary_free.argtypes = [ctypes.c_void_p]
        lib.mib_dictionary_free.restype = None
        lib.mib_dictionary_size.argtypes = [ctypes.c_void_p]
        lib.mib_dictionary_size.restype = ctypes.c_uint64
        lib.mib_encode_batch_dictionary.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Opts),
                                                    ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
        lib.mib_decode_batch_dictionary.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
        if hasattr(lib, 'mib_encoder_new_dictionary'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_encoder_new_dictionary.argtypes = [ctypes.POINTER(_Opts), ctypes.c_void_p]
            lib.mib_encoder_new_dictionary.restype = ctypes.c_void_p
            lib.mib_decoder_new_dictionary.argtypes = [ctypes.POINTER(_DecOpts), ctypes.c_void_p]
            lib.mib_decoder_new_dictionary.restype = ctypes.c_void_p
        lib.mib_encode_batch_n.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Opts), ctypes.c_int,
                                           ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
        lib.mib_decode_batch_n.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_Buf),
                                           ctypes.POINTER(ctypes.c_int)]
        lib.mib_ctx_new.argtypes = [ctypes.c_int]
        lib.mib_ctx_new.restype = ctypes.c_void_p
        lib.mib_ctx_free.argtypes = [ctypes.c_void_p]
        lib.mib_ctx_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Opts), ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_void_p,
                                       ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        lib.mib_ctx_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        lib.mib_ctx_kernel_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(_KTime), ctypes.c_int]
        lib.mib_ctx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.mib_woff2_transform_glyf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
        lib.mib_woff2_transform_hmtx.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
        lib.mib_woff2_reconstruct_glyf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Buf),
                                                   ctypes.POINTER(_Buf)]
        lib.mib_woff2_reconstruct_hmtx.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                                   ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_woff2_decode'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_woff2_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
            lib.mib_debug_sfnt_assemble.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                    ctypes.POINTER(_Span), ctypes.c_char_p, ctypes.c_size_t,
                                                    ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_woff2_decode_batch'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_woff2_decode_batch.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Buf),
                                                   ctypes.POINTER(ctypes.c_int)]
            lib.mib_force_woff2_group_bytes.argtypes = [ctypes.c_uint64]
            lib.mib_force_woff2_group_bytes.restype = None
            lib.mib_debug_sfnt_assemble_batch.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_Span),
                                                          ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
            lib.mib_woff2_batch_last_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
            lib.mib_woff2_batch_last_ms.restype = None
        if hasattr(lib, 'mib_debug_ttc_assemble'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_ttc_assemble.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_Span),
                                                   ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                                                   ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                   ctypes.c_size_t, ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_woff2_encode'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_woff2_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Woff2EncOpts),
                                             ctypes.POINTER(_Buf)]
            lib.mib_woff2_encode_batch.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Woff2EncOpts),
                                                   ctypes.POINTER(_Buf), ctypes.POINTER(ctypes.c_int)]
        if hasattr(lib, 'mib_debug_tables_equal'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_tables_equal.argtypes = [ctypes.POINTER(_Span), ctypes.POINTER(_Span), ctypes.c_char_p,
                                                   ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8)]
        lib.mib_part_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        if hasattr(lib, 'mib_debug_in_place'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_in_place.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
            lib.mib_debug_in_place.restype = None
        if hasattr(lib, 'mib_debug_match_records'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_match_records.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Opts),
                                                    ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_debug_match_passes'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_match_passes.argtypes = [ctypes.POINTER(_Span), ctypes.c_size_t, ctypes.POINTER(_Opts), ctypes.c_int,
                                                   ctypes.c_uint32, ctypes.POINTER(_Buf)]
        if hasattr(lib, 'mib_debug_prefix_codes'):   # (a BROTLI_AMD_LIB build may predate it)
            lib.mib_debug_prefix_codes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(_Buf)]
        lib.mib_default_ctx.restype = ctypes.c_void_p
        lib.mib_ctx_clear_times.argtypes = [ctypes.c_void_p]
        lib.mib_set_allocator.argtypes = [_ALLOC_FN, _FREE_FN, ctypes.c_void_p]
        lib.mib_set_allocator(_alloc_cb, _free_cb, None)
        _lib = lib
    return _lib


def _err(code, what=''):
    msg = _L().mib_strerror(code).decode()
    return BrotliError(msg, code)


def _take(buf):
    addr = ctypes.cast(buf.data, ctypes.c_void_p).value
    b = _results.pop(addr, None) if addr else None
    if b is None:
        return b''
    buf.data = None
    return b if len(b) == buf.size else b[:buf.size]


def _opts(options):
    """option clamping of encode.ts:54-71 / BrotliEncoder constructor :293-310; plus the
    extension `customDictionary` (the encoder side of brotliDecode's option of that name:
    the stream then decodes with, and only with, the same dictionary).  The dictionary's
    bytes object is kept on the returned structure for the duration of the call."""
    options = options or {}
    o = _Opts(11, 22, EncoderMode.GENERIC, 0, None, 0, 0)
    if options.get('quality') is not None:
        o.quality = max(0, min(11, int(options['quality'])))
    if options.get('lgwin') is not None:
        o.lgwin = max(10, min(24, int(options['lgwin'])))
    if options.get('mode') is not None:
        o.mode = int(options['mode'])
    if options.get('sizeHint') is not None:
        o.size_hint = int(options['sizeHint'])
    if options.get('streamChunk') is not None:   # BrotliEncoder throughput mode (brotli_amd.h)
        o.stream_chunk = max(0, int(options['streamChunk']))
    if options.get('customDictionary') is not None:
        d = _bytes(options['customDictionary'])
        o._keep = d
        o.dict, o.dict_len = d, len(d)
    return o


def _in(x):
    """(argument, length, keep-alive) for an input buffer, without copying it: bytes as is,
    any other C-contiguous buffer (bytearray, memoryview slices, numpy, array) by address."""
    if isinstance(x, bytes):
        return x, len(x), x
    try:
        mv = memoryview(x)
    except TypeError:
        b = bytes(bytearray(x))
        return b, len(b), b
    if not mv.c_contiguous:
        b = mv.tobytes()
        return b, len(b), b
    import numpy as np
    a = np.frombuffer(mv.cast('B') if mv.format != 'B' or mv.ndim != 1 else mv, dtype=np.uint8)
    if a.size == 0:
        return b'', 0, a
    return ctypes.c_char_p(a.ctypes.data), a.size, a


def _addr(arg):
    return ctypes.cast(arg if isinstance(arg, ctypes.c_char_p) else ctypes.c_char_p(arg), ctypes.c_void_p)


def _bytes(x):
    """Uint8Array / Int8Array equivalents: any buffer (bytes, bytearray, memoryview, array('b'),
    numpy int8/uint8) is taken as its raw bytes, as decode.ts:31-33 views an Int8Array."""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    try:
        return bytes(memoryview(x).cast('B'))
    except TypeError:
        return bytes(bytearray(x))


class Dictionary:
    """A prepared dictionary (mib_dictionary, brotli_amd.h): bytes that many small, similar
    buffers are compressed against, uploaded and indexed on the GPU once.  Pass it as
    `dictionary=` to encode_batch / decode_batch or as options['dictionary'] to brotliEncode /
    brotliDecode / BrotliEncoder / BrotliDecoder.  Copies may come from anywhere in it, so a
    stream written with one decodes only with one (of the same bytes).  close() drops this
    object's reference: the object must stay open while a one-shot call uses it and may not be
    given to a new call or session afterwards, but the sessions already made with it hold
    references of their own and keep working -- the device memory goes with the last of them.
    len() is the dictionary's size."""

    def __init__(self, data):
        d = _bytes(data)
        h = ctypes.c_void_p()
        rc = _L().mib_dictionary_new(d, len(d), ctypes.byref(h))
        if rc:
            raise _err(rc)
        self._h = h.value
        self._n = len(d)

    def __len__(self):
        return self._n

    @property
    def closed(self):
        return self._h is None

    def close(self):
        if getattr(self, '_h', None):
            _L().mib_dictionary_free(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown)
            pass


def _dictionary(dictionary, options):
    """the handle of a `dictionary` argument; both kinds of dictionary at once is an error
    (checked before the library is loaded: no device needed to be told)"""
    if not isinstance(dictionary, Dictionary):
        raise TypeError('dictionary must be a brotli_amd.Dictionary')
    if isinstance(options, dict) and options.get('customDictionary') is not None:
        raise ValueError('dictionary and customDictionary exclude each other')
    if dictionary.closed:
        raise ValueError('the Dictionary is closed')
    return dictionary._h


def brotliEncode(input, options=None):
    if options and options.get('dictionary') is not None:   # the batch with k = 1
        return encode_batch([input], options, dictionary=options['dictionary'])[0]
    data, n, _keep = _in(input)
    buf = _Buf()
    rc = _L().mib_encode(data, n, ctypes.byref(_opts(options)), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


class BrotliEncoder:
    """Streaming encoder: update() returns the newly completed bytes, finish() the rest.
    options['dictionary'] (a Dictionary; not with 'customDictionary'): the session copies from
    anywhere in the prepared dictionary, in place on the device, and holds a reference to it --
    its stream decodes through decode_batch(dictionary=) and BrotliDecoder({'dictionary': ...})."""

    def __init__(self, options=None):
        self._dictionary = None
        if isinstance(options, dict) and options.get('dictionary') is not None:
            h = _dictionary(options['dictionary'], options)
            self._dictionary = options['dictionary']
            self._h = _L().mib_encoder_new_dictionary(ctypes.byref(_opts(options)), h)
        else:
            self._h = _L().mib_encoder_new(ctypes.byref(_opts(options)))
        if not self._h:
            raise BrotliError('brotli_amd: encoder creation failed')

    def update(self, chunk):
        data, n, _keep = _in(chunk)
        buf = _Buf()
        rc = _L().mib_encoder_update(self._h, data, n, ctypes.byref(buf))
        if rc:
            raise _err(rc)
        return _take(buf)

    def finish(self):
        buf = _Buf()
        rc = _L().mib_encoder_finish(self._h, ctypes.byref(buf))
        if rc:
            raise _err(rc)
        return _take(buf)

    def __del__(self):
        if getattr(self, '_h', None):
            _L().mib_encoder_free(self._h)
            self._h = None


def encoder_update_batch(encoders, chunks):
    """Advance independent BrotliEncoders by one chunk each in one GPU launch sequence;
    returns each encoder's update() result.  The encoders may hold different dictionaries
    (options['dictionary'], 'customDictionary') or none: each chunk is searched against its own."""
    k = len(encoders)
    keep = [_in(b) for b in chunks]
    hs = (ctypes.c_void_p * k)(*[e._h for e in encoders])
    spans = (_Span * k)(*[_Span(_addr(a), n) for a, n, _ in keep])
    outs = (_Buf * k)()
    rc = _L().mib_encoder_update_batch(hs, spans, k, outs)
    if rc:
        raise _err(rc)
    return [_take(outs[i]) for i in range(k)]


def brotliDecodedSize(data):
    data, n, _keep = _in(data)
    return int(_L().mib_decoded_size(data, n))


def brotliDecode(buffer, options=None):
    """decode.ts:18-65: options = {'maxOutputSize', 'customDictionary'} or a legacy int size."""
    if isinstance(options, dict) and options.get('dictionary') is not None:   # the batch with k = 1
        r = decode_batch([buffer], dictionary=options['dictionary'], options=options)[0]
        if isinstance(r, BrotliError):
            raise r
        return r
    data, n, _keep = _in(buffer)
    exact, max_out, dic = -1, -1, None
    if isinstance(options, int) and not isinstance(options, bool):
        exact = options
    elif options:
        if options.get('maxOutputSize') is not None:
            max_out = int(options['maxOutputSize'])
        if options.get('customDictionary') is not None:
            dic = _bytes(options['customDictionary'])
    buf = _Buf()
    rc = _L().mib_decode(data, n, dic, len(dic) if dic is not None else 0, max_out, exact, ctypes.byref(buf))
    if rc == -103:   # MIB_E_OUTPUT_LIMIT: the reference's wrapper message
        raise BrotliError('Decompressed size %d exceeds limit %d' % (buf.size, max_out), rc)
    if rc:
        raise _err(rc)
    return _take(buf)


class BrotliDecoder:
    """Streaming decoder (extension: the reference decodes in one shot only).  update(chunk)
    takes the next bytes of one stream, cut anywhere, and returns the bytes they complete;
    finish() declares the input ended and returns the rest, raising the reference decoder's
    error for an incomplete stream; `finished` is true once the last metablock is decoded.
    options: {'customDictionary', 'maxOutputSize' (total), 'outWindow' (output bytes per device
    pass, default 16 MiB, 64 KiB .. 512 MiB), 'dictionary' (a Dictionary, not with
    'customDictionary': copies from anywhere in it are valid, as in decode_batch(dictionary=);
    the session reads it in place and holds a reference)}.  Bytes behind the stream's end raise code -17;
    after an error every call raises it again."""

    def __init__(self, options=None):
        options = options or {}
        self._dictionary = None
        handle = None
        if options.get('dictionary') is not None:
            handle = _dictionary(options['dictionary'], options)
            self._dictionary = options['dictionary']
        o = _DecOpts(None, 0, -1, 0)
        if options.get('customDictionary') is not None:
            d = _bytes(options['customDictionary'])
            o.dict, o.dict_len = d, len(d)
        if options.get('maxOutputSize') is not None:
            o.max_out = max(0, int(options['maxOutputSize']))
        if options.get('outWindow') is not None:
            o.out_window = max(0, int(options['outWindow']))
        self._max_out = o.max_out
        if handle is not None:
            self._h = _L().mib_decoder_new_dictionary(ctypes.byref(o), handle)
        else:
            self._h = _L().mib_decoder_new(ctypes.byref(o))
        if not self._h:
            raise BrotliError('brotli_amd: decoder creation failed')

    def _result(self, rc, buf):
        if rc == -103:
            raise BrotliError('Decompressed size %d exceeds limit %d' % (buf.size, self._max_out), rc)
        if rc:
            raise _err(rc)
        return _take(buf)

    def update(self, chunk):
        data, n, _keep = _in(chunk)
        buf = _Buf()
        return self._result(_L().mib_decoder_update(self._h, data, n, ctypes.byref(buf)), buf)

    def finish(self):
        buf = _Buf()
        return self._result(_L().mib_decoder_finish(self._h, ctypes.byref(buf)), buf)

    @property
    def finished(self):
        return bool(_L().mib_decoder_is_finished(self._h))

    def _stats(self):
        p, r = ctypes.c_uint64(), ctypes.c_uint64()
        _L().mib_decoder_stats(self._h, ctypes.byref(p), ctypes.byref(r))
        return int(p.value), int(r.value)

    @property
    def passes(self):
        """diagnostic (tests): device passes made so far"""
        return self._stats()[0]

    @property
    def redecoded(self):
        """diagnostic: output bytes decoded more than once so far"""
        return self._stats()[1]

    @property
    def held_output(self):
        """decoded bytes not yet handed out (a device-resident call's range was full)"""
        return int(_L().mib_decoder_held_output(self._h))

    def __del__(self):
        if getattr(self, '_h', None):
            _L().mib_decoder_free(self._h)
            self._h = None


def _decoder_batch_results(decoders, rc, outs, st):
    if rc:
        raise _err(rc)
    res = []
    for i, d in enumerate(decoders):
        try:
            res.append(d._result(st[i], outs[i]))
        except BrotliError as e:
            res.append(e)
    return res


def decoder_update_batch(decoders, chunks):
    """Advance many BrotliDecoder sessions by one chunk each: a round is one decode launch over
    every session that still has work (mib_decoder_update_batch).  Returns a list with, per
    slot, the bytes decoder.update(chunk) alone would have returned, or the BrotliError it would
    have raised (not raised here: the other sessions go on).  The decoders must be distinct;
    they may hold different dictionaries (options['dictionary'], 'customDictionary') or none."""
    k = len(decoders)
    if len(chunks) != k:
        raise ValueError('decoder_update_batch: %d decoders, %d chunks' % (k, len(chunks)))
    keep = [_in(b) for b in chunks]
    hs = (ctypes.c_void_p * k)(*[d._h for d in decoders])
    spans = (_Span * k)(*[_Span(_addr(a) if n else None, n) for a, n, _ in keep])
    outs = (_Buf * k)()
    st = (ctypes.c_int * k)()
    return _decoder_batch_results(decoders, _L().mib_decoder_update_batch(hs, spans, k, outs, st), outs, st)


def decoder_finish_batch(decoders):
    """finish() of many BrotliDecoder sessions in shared launches (mib_decoder_finish_batch):
    per slot the rest of the output, or the BrotliError of an incomplete stream."""
    k = len(decoders)
    hs = (ctypes.c_void_p * k)(*[d._h for d in decoders])
    outs = (_Buf * k)()
    st = (ctypes.c_int * k)()
    return _decoder_batch_results(decoders, _L().mib_decoder_finish_batch(hs, k, outs, st), outs, st)


MORE_OUTPUT = 1   # MIB_DEC_MORE_OUTPUT: the slot's output range is full, the session has more


def _device_offsets(what, offsets, k):
    if len(offsets) != k + 1:
        raise ValueError('%s: %d decoders need %d offsets, got %d' % (what, k, k + 1, len(offsets)))
    return (ctypes.c_uint64 * (k + 1))(*offsets)


def decoder_update_batch_device(decoders, d_in, in_offsets, d_out, out_offsets):
    """decoder_update_batch with the chunks and the decoded bytes in device memory
    (mib_decoder_update_batch_device): d_in / d_out are raw device pointers (tensor.data_ptr()) on
    the default device, session i's chunk is d_in[in_offsets[i]:in_offsets[i+1]] and its bytes
    go to d_out[out_offsets[i]:out_offsets[i+1]].  Returns (sizes, statuses): per slot the bytes
    written and 0, MORE_OUTPUT (the range is full and the session has more: call again, empty
    chunks will do) or the session's negative error code -- a value, not raised."""
    k = len(decoders)
    ioff = _device_offsets('decoder_update_batch_device', in_offsets, k)
    ooff = _device_offsets('decoder_update_batch_device', out_offsets, k)
    hs = (ctypes.c_void_p * k)(*[d._h for d in decoders])
    sizes = (ctypes.c_uint64 * k)()
    st = (ctypes.c_int * k)()
    rc = _L().mib_decoder_update_batch_device(hs, d_in, ioff, k, d_out, ooff, sizes, st)
    if rc:
        raise _err(rc)
    return list(sizes), list(st)


def decoder_finish_batch_device(decoders, d_out, out_offsets):
    """decoder_finish_batch into device memory (mib_decoder_finish_batch_device); returns
    (sizes, statuses) as decoder_update_batch_device does."""
    k = len(decoders)
    ooff = _device_offsets('decoder_finish_batch_device', out_offsets, k)
    hs = (ctypes.c_void_p * k)(*[d._h for d in decoders])
    sizes = (ctypes.c_uint64 * k)()
    st = (ctypes.c_int * k)()
    rc = _L().mib_decoder_finish_batch_device(hs, k, d_out, ooff, sizes, st)
    if rc:
        raise _err(rc)
    return list(sizes), list(st)


def debug_copy_batch(srcs, dsts, sizes):
    """Diagnostic (tests): the device calls' copy kernel alone (mib_debug_copy_batch): copy i moves
    sizes[i] bytes from the device address srcs[i] to the device address dsts[i]."""
    k = len(sizes)
    rc = _L().mib_debug_copy_batch((ctypes.c_void_p * k)(*srcs), (ctypes.c_void_p * k)(*dsts), (ctypes.c_uint64 * k)(*sizes), k)
    if rc:
        raise _err(rc)


def encode_batch(buffers, options=None, gpus=None, dictionary=None):
    """Encode independent buffers in one GPU launch sequence; returns list of bytes.  gpus:
    shard the batch over that many GPUs (0: every visible one; mib_encode_batch_n).
    dictionary: a Dictionary every buffer is compressed against (mib_encode_batch_dictionary;
    not with gpus, not with options['customDictionary'])."""
    k = len(buffers)
    keep = [_in(b) for b in buffers]
    spans = (_Span * k)(*[_Span(_addr(a), n) for a, n, _ in keep])
    outs = (_Buf * k)()
    st = (ctypes.c_int * k)()
    if dictionary is not None:
        if gpus is not None:
            raise ValueError('a Dictionary lives on one GPU: not with gpus')
        rc = _L().mib_encode_batch_dictionary(spans, k, ctypes.byref(_opts(options)), _dictionary(dictionary, options), outs, st)
    elif gpus is None:
        rc = _L().mib_encode_batch(spans, k, ctypes.byref(_opts(options)), outs, st)
    else:
        rc = _L().mib_encode_batch_n(spans, k, ctypes.byref(_opts(options)), int(gpus), outs, st)
    if rc:
        raise _err(rc)
    res = [_take(outs[i]) for i in range(k)]
    for i in range(k):
        if st[i]:
            raise _err(st[i])
    return res


def debug_dp_launches():
    """Diagnostic (tests): this process's launches of the parse's kernel so far, by pieces a
    wave: {1: n, 2: n, 4: n, 8: n} (mib_debug_dp_launches)."""
    out = (ctypes.c_uint64 * 4)()
    _L().mib_debug_dp_launches(out)
    return {1: out[0], 2: out[1], 4: out[2], 8: out[3]}


def debug_match_records(buffers, options=None, passes=0, history=0):
    """Diagnostic (tests): the records the encoder's match search gives a batch of buffers, pass
    by pass (mib_debug_match_passes): the bucket sort and the candidate walk, then the passes of
    the bit set `passes` where an encode call with these options runs them -- 1 the near scan, 2
    static-dictionary words, 4 the tail copies of options['customDictionary'].  The first
    `history` bytes of every buffer lie before its stream (a streaming chunk's window).  Per
    buffer a numpy uint32 array of shape (len(buffer) - history, entries), each entry
    length << 24 | distance, valid ones first, 0 after (include/brotli_amd.h has the formats)."""
    import numpy as np
    k = len(buffers)
    keep = [_in(b) for b in buffers]
    spans = (_Span * k)(*[_Span(_addr(a), n) for a, n, _ in keep])
    outs = (_Buf * k)()
    if passes or history:
        rc = _L().mib_debug_match_passes(spans, k, ctypes.byref(_opts(options)), int(passes), int(history), outs)
    else:
        rc = _L().mib_debug_match_records(spans, k, ctypes.byref(_opts(options)), outs)
    if rc:
        raise _err(rc)
    res = []
    for i in range(k):
        n = keep[i][1] - history
        a = np.frombuffer(_take(outs[i]), dtype='<u4')
        res.append(a.reshape(n, -1) if n else a.reshape(0, 4))
    return res


def debug_prefix_codes(histograms):
    """Diagnostic (tests): the encoder's Huffman kernel alone on chosen histograms
    (mib_debug_prefix_codes).  histograms: sequences of 256 (literal), 704 (command) or 64
    (distance) counts.  Per histogram a dict: 'bits' (the serialised code's bit count), 'depths'
    and 'codes' (lists over the alphabet) and 'bytes' (the 1024 bytes it was serialised into)."""
    import numpy as np
    k = len(histograms)
    hs = [np.ascontiguousarray(np.asarray(h, dtype='<u4')) for h in histograms]
    alpha = np.array([len(h) for h in hs], dtype='<u4')
    flat = np.ascontiguousarray(np.concatenate(hs)) if k else np.zeros(0, '<u4')
    out = _Buf()
    rc = _L().mib_debug_prefix_codes(flat.ctypes.data, alpha.ctypes.data, k, ctypes.byref(out))
    if rc:
        raise _err(rc)
    raw = _take(out)
    rec = 4 + 704 + 2 * 704 + 1024   # MIB_PREFIX_CODE_RECORD
    res = []
    for i in range(k):
        r, n = raw[i * rec:(i + 1) * rec], len(hs[i])
        res.append({'bits': int.from_bytes(r[:4], 'little'), 'depths': list(r[4:4 + n]),
                    'codes': np.frombuffer(r, dtype='<u2', count=n, offset=4 + 704).tolist(),
                    'bytes': bytes(r[4 + 704 + 2 * 704:])})
    return res


def decode_batch(buffers, gpus=None, dictionary=None, options=None):
    """Decode independent streams on the GPU; returns a list of bytes or BrotliError.  gpus:
    shard the batch over that many GPUs (0: every visible one; mib_decode_batch_n).
    dictionary: the Dictionary the streams were written with (mib_decode_batch_dictionary; not
    with gpus); with it options may hold 'maxOutputSize', which applies to every stream."""
    k = len(buffers)
    keep = [_in(b) for b in buffers]
    spans = (_Span * k)(*[_Span(_addr(a), n) for a, n, _ in keep])
    outs = (_Buf * k)()
    st = (ctypes.c_int * k)()
    if dictionary is not None:
        if gpus is not None:
            raise ValueError('a Dictionary lives on one GPU: not with gpus')
        max_out = -1
        if isinstance(options, dict) and options.get('maxOutputSize') is not None:
            max_out = int(options['maxOutputSize'])
        rc = _L().mib_decode_batch_dictionary(spans, k, _dictionary(dictionary, options), max_out, outs, st)
        if rc:
            raise _err(rc)
        res = []
        for i in range(k):
            if st[i] == -103:   # MIB_E_OUTPUT_LIMIT: brotliDecode's message
                res.append(BrotliError('Decompressed size %d exceeds limit %d' % (outs[i].size, max_out), st[i]))
            else:
                res.append(_take(outs[i]) if st[i] == 0 else _err(st[i]))
        return res
    if options is not None:
        raise ValueError('options apply to a call with a dictionary only')
    if gpus is None:
        rc = _L().mib_decode_batch(spans, k, outs, st)
    else:
        rc = _L().mib_decode_batch_n(spans, k, int(gpus), outs, st)
    if rc:
        raise _err(rc)
    return [(_take(outs[i]) if st[i] == 0 else _err(st[i])) for i in range(k)]


def woff2_transform_glyf(ttf):
    """The WOFF2-transformed 'glyf' table of a TrueType font (W3C WOFF2 section 5.1), computed on
    the GPU: the FONT-mode input of brotliEncode for a WOFF2 writer (reference README.md:63)."""
    data = _bytes(ttf)
    buf = _Buf()
    rc = _L().mib_woff2_transform_glyf(data, len(data), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def woff2_transform_hmtx(ttf):
    """The WOFF2-transformed 'hmtx' table (W3C WOFF2 section 5.4), computed on the GPU, or None
    when no transform applies (both side-bearing arrays differ from the glyphs' xMin)."""
    data = _bytes(ttf)
    buf = _Buf()
    rc = _L().mib_woff2_transform_hmtx(data, len(data), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    if not buf.size:
        _L().mib_buf_free(ctypes.byref(buf))
        return None
    return _take(buf)


def woff2_reconstruct_glyf(data):
    """(glyf, loca): the TrueType tables a WOFF2-transformed 'glyf' table stands for (W3C WOFF2
    sections 5.1, 5.3), computed on the GPU, byte for byte as fontTools reconstructs and compiles
    them (4-byte padding; loca in the header's indexFormat).  The input is untrusted: a table
    that does not parse raises BrotliError (MIB_E_INVALID_ARG)."""
    data = _bytes(data)
    glyf, loca = _Buf(), _Buf()
    rc = _L().mib_woff2_reconstruct_glyf(data, len(data), ctypes.byref(glyf), ctypes.byref(loca))
    if rc:
        raise _err(rc)
    return _take(glyf), _take(loca)


def woff2_reconstruct_hmtx(data, glyf, loca, num_glyphs, num_hmetrics):
    """The 'hmtx' table of a WOFF2-transformed one (section 5.4), computed on the GPU: the side
    bearings the transform dropped are the glyphs' xMin in `glyf` / `loca` (as
    woff2_reconstruct_glyf returns them)."""
    data, glyf, loca = _bytes(data), _bytes(glyf), _bytes(loca)
    if not 0 <= int(num_glyphs) <= 0xFFFFFFFF or not 0 <= int(num_hmetrics) <= 0xFFFFFFFF:
        raise _err(-101)   # MIB_E_INVALID_ARG
    buf = _Buf()
    rc = _L().mib_woff2_reconstruct_hmtx(data, len(data), glyf, len(glyf), loca, len(loca), int(num_glyphs),
                                         int(num_hmetrics), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def woff2_decode(data):
    """The sfnt a .woff2 file (W3C WOFF2) stands for: the Brotli stream decoded, glyf, loca and
    hmtx reconstructed and the font assembled on the GPU -- records sorted by tag, tables in the
    file's order at 4-byte boundaries, checksums and head's checkSumAdjustment computed.  A font
    collection (flavor ttcf) gives its TTC: the header, the members' directories back to back,
    then every table that a member lists, once; a shared table has one checksum, and a shared
    head carries the checkSumAdjustment of the last member that lists it.
    The file is untrusted: one that does not parse raises BrotliError (MIB_E_INVALID_ARG, or the
    decoder's code for a corrupt Brotli stream)."""
    data = _bytes(data)
    buf = _Buf()
    rc = _L().mib_woff2_decode(data, len(data), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def debug_sfnt_assemble(flavor, tables, misalign=None):
    """Diagnostic (tests): woff2_decode's assembly kernels alone over [(tag, bytes)], tags of four
    bytes; misalign[i] in 0..15 is the misalignment table i's bytes get in device memory (None:
    packed back to back)."""
    tables = [(bytes(tag), _bytes(data)) for tag, data in tables]
    k = len(tables)
    if any(len(tag) != 4 for tag, _ in tables) or (misalign is not None and len(misalign) != k):
        raise _err(-101)   # MIB_E_INVALID_ARG
    tags = (ctypes.c_uint32 * max(k, 1))(*[int.from_bytes(tag, 'big') for tag, _ in tables])
    keep = [ctypes.create_string_buffer(data, len(data)) for _, data in tables]
    spans = (_Span * max(k, 1))()
    for i, b in enumerate(keep):
        spans[i].data = ctypes.cast(b, ctypes.c_void_p).value
        spans[i].size = len(tables[i][1])
    mis = bytes(misalign) if misalign is not None else None
    buf = _Buf()
    rc = _L().mib_debug_sfnt_assemble(int(flavor) & 0xFFFFFFFF, tags, spans, mis, k, ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def woff2_decode_batch(files):
    """woff2_decode of many files in shared launches (mib_woff2_decode_batch): the Brotli streams
    decode in one launch and the sfnts are assembled in one.  Returns a list with, per slot, the
    bytes woff2_decode(file) alone would have returned, or the BrotliError it would have raised
    (not raised here: the other files go on).  The same file may stand in several slots, and a
    collection in any slot beside single fonts."""
    keep = [_in(b) for b in files]
    k = len(keep)
    spans = (_Span * max(k, 1))(*[_Span(_addr(a) if n else None, n) for a, n, _ in keep])
    outs = (_Buf * max(k, 1))()
    st = (ctypes.c_int * max(k, 1))()
    rc = _L().mib_woff2_decode_batch(spans, k, outs, st)
    if rc:
        raise _err(rc)
    return [_err(st[i]) if st[i] else _take(outs[i]) for i in range(k)]


def _woff2_enc_opts(options):
    """quality and lgwin clamped as brotliEncode's; transformGlyf / transformHmtx default to True;
    `transforms` (the C ABI's bit set, MIB_WOFF2_GLYF 1 | MIB_WOFF2_HMTX 2) overrides both."""
    options = options or {}
    o = _Woff2EncOpts(11, 22, 0)
    if options.get('quality') is not None:
        o.quality = max(0, min(11, int(options['quality'])))
    if options.get('lgwin') is not None:
        o.lgwin = max(10, min(24, int(options['lgwin'])))
    if options.get('transforms') is not None:
        o.transforms = int(options['transforms']) & 0xFFFFFFFF
    else:
        o.transforms = (1 if options.get('transformGlyf', True) else 0) | (2 if options.get('transformHmtx', True) else 0)
    return o


def woff2_encode(sfnt, options=None):
    """The .woff2 file (W3C WOFF2) of a single-font sfnt, written on the GPU: glyf, loca and hmtx
    transformed, the other tables copied beside them, the stream compressed in FONT mode
    (mib_woff2_encode).  options: quality, lgwin, transformGlyf, transformHmtx.  Every byte but the
    Brotli stream is fixed (tables in tag order, DSIG dropped); woff2_decode reads every file
    written.  A font that does not parse, or that the glyf transform rejects, raises BrotliError
    (MIB_E_INVALID_ARG).
    An OpenType collection (TTC) becomes the .woff2 file of flavor ttcf: every table once in one
    directory -- tables of one tag, offset and length, and tables of one tag and length whose bytes
    the device finds equal, are one entry; glyf and loca are shared as a pair -- and each member's
    index list in the CollectionHeader."""
    data = _bytes(sfnt)
    buf = _Buf()
    rc = _L().mib_woff2_encode(data, len(data), ctypes.byref(_woff2_enc_opts(options)), ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def woff2_encode_batch(sfnts, options=None):
    """woff2_encode of many fonts in shared launches (mib_woff2_encode_batch): one upload, one copy
    launch and one encode call per group of fonts.  Returns a list with, per slot, the file or the
    BrotliError woff2_encode(font) alone would have raised (not raised here: the other fonts go
    on).  The same font may stand in several slots, and a collection in any slot beside single
    fonts (it is one file and one stream of its group)."""
    keep = [_in(b) for b in sfnts]
    k = len(keep)
    spans = (_Span * max(k, 1))(*[_Span(_addr(a) if n else None, n) for a, n, _ in keep])
    outs = (_Buf * max(k, 1))()
    st = (ctypes.c_int * max(k, 1))()
    rc = _L().mib_woff2_encode_batch(spans, k, ctypes.byref(_woff2_enc_opts(options)), outs, st)
    if rc:
        raise _err(rc)
    return [_err(st[i]) if st[i] else _take(outs[i]) for i in range(k)]


def debug_tables_equal(pairs, misalign_a=None, misalign_b=None):
    """Diagnostic (tests): the collection writer's compare kernel alone over pairs = [(a, b)], byte
    strings of one length each; misalign_a[i] / misalign_b[i] in 0..15 are the misalignments the
    two sides get in device memory (None: 0).  Returns [bool]: True where a and b are equal."""
    pairs = [(_bytes(a), _bytes(b)) for a, b in pairs]
    k = len(pairs)
    if any(m is not None and len(m) != k for m in (misalign_a, misalign_b)):
        raise _err(-101)   # MIB_E_INVALID_ARG
    keep = [(ctypes.create_string_buffer(a, len(a)), ctypes.create_string_buffer(b, len(b))) for a, b in pairs]
    sa, sb = (_Span * max(k, 1))(), (_Span * max(k, 1))()
    for i, (a, b) in enumerate(keep):
        sa[i].data, sa[i].size = ctypes.cast(a, ctypes.c_void_p).value, len(pairs[i][0])
        sb[i].data, sb[i].size = ctypes.cast(b, ctypes.c_void_p).value, len(pairs[i][1])
    differ = (ctypes.c_uint8 * max(k, 1))(*([2] * max(k, 1)))
    rc = _L().mib_debug_tables_equal(sa, sb, bytes(misalign_a) if misalign_a is not None else None,
                                     bytes(misalign_b) if misalign_b is not None else None, k, differ)
    if rc:
        raise _err(rc)
    return [differ[i] == 0 for i in range(k)]


def force_woff2_group_bytes(n):
    """Diagnostic (tests): woff2_decode_batch works its files in groups whose decompressed streams
    sum to at most n bytes (0: the default); a larger file is a group alone."""
    _L().mib_force_woff2_group_bytes(int(n))


def woff2_batch_last_ms():
    """Diagnostic (measurements): (the per-font glyf reconstruct loops, the whole call) of the last
    woff2_decode_batch or woff2_decode (which is the batch with one file) that reached the device,
    host wall time in ms."""
    out = (ctypes.c_double * 2)()
    _L().mib_woff2_batch_last_ms(out)
    return out[0], out[1]


def debug_sfnt_assemble_batch(fonts, misalign=None):
    """Diagnostic (tests): woff2_decode_batch's assembly kernels alone over fonts =
    [(flavor, [(tag, bytes)])]; misalign: per font None or a list as debug_sfnt_assemble takes
    (None: every font packed back to back).  Returns the list of sfnts."""
    fonts = [(int(flavor) & 0xFFFFFFFF, [(bytes(tag), _bytes(data)) for tag, data in tables]) for flavor, tables in fonts]
    k = len(fonts)
    flat = [t for _, tables in fonts for t in tables]
    n = len(flat)
    if any(len(tag) != 4 for tag, _ in flat) or (misalign is not None and len(misalign) != k):
        raise _err(-101)   # MIB_E_INVALID_ARG
    mis = None
    if misalign is not None:
        per = [list(m) if m is not None else [0] * len(tables) for m, (_, tables) in zip(misalign, fonts)]
        if any(len(m) != len(tables) for m, (_, tables) in zip(per, fonts)):
            raise _err(-101)
        mis = bytes(v for m in per for v in m)
    flavors = (ctypes.c_uint32 * max(k, 1))(*[f for f, _ in fonts])
    counts = (ctypes.c_uint32 * max(k, 1))(*[len(tables) for _, tables in fonts])
    tags = (ctypes.c_uint32 * max(n, 1))(*[int.from_bytes(tag, 'big') for tag, _ in flat])
    blob = b''.join(data for _, data in flat)
    keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
    base = ctypes.addressof(keep)
    spans = (_Span * max(n, 1))()
    at = 0
    for i, (_, data) in enumerate(flat):
        spans[i].data = base + at
        spans[i].size = len(data)
        at += len(data)
    outs = (_Buf * max(k, 1))()
    rc = _L().mib_debug_sfnt_assemble_batch(flavors, counts, tags, spans, mis, k, outs)
    if rc:
        raise _err(rc)
    return [_take(outs[i]) for i in range(k)]


def debug_ttc_assemble(version, tables, fonts, misalign=None):
    """Diagnostic (tests): woff2_decode's assembly kernels alone over a collection: tables =
    [(tag, bytes)], its directory (tags may repeat); fonts = [(flavor, [index, ...])], each
    member's tables by their indices; misalign as debug_sfnt_assemble takes it.  Returns the TTC."""
    tables = [(bytes(tag), _bytes(data)) for tag, data in tables]
    fonts = [(int(flavor) & 0xFFFFFFFF, [int(i) for i in idx]) for flavor, idx in fonts]
    k, nf = len(tables), len(fonts)
    flat = [i for _, idx in fonts for i in idx]
    if any(len(tag) != 4 for tag, _ in tables) or (misalign is not None and len(misalign) != k) or \
            any(i < 0 or i > 0xFFFFFFFF for i in flat):
        raise _err(-101)   # MIB_E_INVALID_ARG
    tags = (ctypes.c_uint32 * max(k, 1))(*[int.from_bytes(tag, 'big') for tag, _ in tables])
    keep = [ctypes.create_string_buffer(data, len(data)) for _, data in tables]
    spans = (_Span * max(k, 1))()
    for i, b in enumerate(keep):
        spans[i].data = ctypes.cast(b, ctypes.c_void_p).value
        spans[i].size = len(tables[i][1])
    mis = bytes(misalign) if misalign is not None else None
    flavors = (ctypes.c_uint32 * max(nf, 1))(*[f for f, _ in fonts])
    counts = (ctypes.c_uint32 * max(nf, 1))(*[len(idx) for _, idx in fonts])
    indices = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
    buf = _Buf()
    rc = _L().mib_debug_ttc_assemble(int(version) & 0xFFFFFFFF, tags, spans, mis, k, flavors, counts, indices, nf,
                                     ctypes.byref(buf))
    if rc:
        raise _err(rc)
    return _take(buf)


def part_stats(ctx=None):
    """(streams decoded part-parallel, of those sent back to the serial decoder) for a
    DeviceContext, or the host API's default context"""
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _L().mib_part_stats(ctx._c if ctx is not None else None, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


IN_PLACE_SLACK = 101   # MIB_IN_PLACE_SLACK: a slot of size + this lets a one-metablock stream decode in place


def in_place_stats(ctx=None):
    """Diagnostic (tests): (streams that finished in their output slots, streams that began there
    and went back to the scratch ring) in the last serial decode launch of a DeviceContext, or
    of the host API's default context (mib_debug_in_place)"""
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _L().mib_debug_in_place(ctx._c if ctx is not None else None, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def _prof_mode(on):
    return 2 if on == 'decode' else (1 if on else 0)


def default_profiling(on=True, clear=True):
    """Per-kernel timing (HIP events) of the host-buffer calls (brotliEncode, brotliDecode,
    BrotliEncoder, the batches): on / off / 'decode' (the decoder's kernels only), and the
    accumulated times cleared unless clear=False."""
    c = _L().mib_default_ctx()
    if not c:
        raise BrotliError('brotli_amd: no usable device')
    _L().mib_ctx_set_profiling(c, _prof_mode(on))
    if clear:
        _L().mib_ctx_clear_times(c)


def default_kernel_times():
    """{kernel: (ms, launches)} accumulated by the host-buffer calls since default_profiling()"""
    c = _L().mib_default_ctx()
    arr = (_KTime * 64)()
    n = _L().mib_ctx_kernel_times(c, arr, 64)
    return {arr[i].name.decode(): (arr[i].ms, arr[i].launches) for i in range(min(n, 64))}


class DeviceContext:
    """Device-resident batches (torch tensors / raw device pointers) for bench and the
    multi-GPU driver; wraps mib_ctx_* of include/brotli_amd.h."""

    def __init__(self, device=0, profiling=False):
        self._c = _L().mib_ctx_new(device)
        if not self._c:
            raise BrotliError('brotli_amd: no usable device %d' % device)
        _L().mib_ctx_set_profiling(self._c, _prof_mode(profiling))

    def set_profiling(self, on):
        """True / False / 'decode' (the decoder's kernels only)."""
        _L().mib_ctx_set_profiling(self._c, _prof_mode(on))

    def close(self):
        if getattr(self, '_c', None) and _lib is not None:
            _lib.mib_ctx_free(self._c)
        self._c = None

    def __del__(self):
        self.close()

    def encode(self, d_in, in_offsets, d_out, out_cap, options=None, stream=None):
        k = len(in_offsets) - 1
        ioff = (ctypes.c_uint64 * (k + 1))(*in_offsets)
        ooff = (ctypes.c_uint64 * (k + 1))()
        rc = _L().mib_ctx_encode(self._c, ctypes.byref(_opts(options)), d_in, ioff, k, d_out, out_cap, ooff, stream)
        if rc:
            raise _err(rc)
        return list(ooff)

    def decode(self, d_in, in_offsets, d_out, out_offsets, stream=None):
        k = len(in_offsets) - 1
        ioff = (ctypes.c_uint64 * (k + 1))(*in_offsets)
        ooff = (ctypes.c_uint64 * (k + 1))(*out_offsets)
        sizes = (ctypes.c_int64 * k)()
        st = (ctypes.c_int * k)()
        rc = _L().mib_ctx_decode(self._c, d_in, ioff, k, d_out, ooff, sizes, st, stream)
        if rc and rc != -104:
            raise _err(rc)
        return list(sizes), list(st)

    def kernel_times(self):
        arr = (_KTime * 32)()
        n = _L().mib_ctx_kernel_times(self._c, arr, 32)
        return {arr[i].name.decode(): (arr[i].ms, arr[i].launches) for i in range(min(n, 32))}
