"""ctypes binding of the ORACLE (oracle/liboracle.so): the CPU restatement of the
reference used as the checker.  Test infrastructure only -- the product never imports it."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'oracle', 'liboracle.so')
_lib = None
_P = ctypes.POINTER(ctypes.c_uint8)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(['make', '-s', '-C', os.path.join(ROOT, 'oracle')], check=True)
        _lib = ctypes.CDLL(LIB)
        _lib.oracle_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_size_t)]
        _lib.oracle_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.c_int64, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_size_t)]
        _lib.oracle_peek_decoded_size.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        _lib.oracle_peek_decoded_size.restype = ctypes.c_int64
    return _lib


def encode(data, quality=11, lgwin=22, mode=0):
    """oracle brotliEncode (ref-fixed); raises on unsupported quality."""
    o, n = _P(), ctypes.c_size_t()
    rc = lib().oracle_encode(data, len(data), quality, lgwin, mode, ctypes.byref(o), ctypes.byref(n))
    if rc:
        raise RuntimeError('oracle_encode rc=%d' % rc)
    r = ctypes.string_at(o, n.value)
    lib().oracle_free(o)
    return r


def bt_matches(data, lgwin=22):
    """per-position findAllMatches lists (pass 1 of the q11 parse): [(i, [(distance, length)...])]"""
    import array
    cap = 8 * len(data) + 64
    buf = (ctypes.c_uint32 * cap)()
    lib().oracle_bt_matches.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    lib().oracle_bt_matches.restype = ctypes.c_int64
    w = lib().oracle_bt_matches(data, len(data), lgwin, buf, cap)
    if w < 0:
        raise RuntimeError('oracle_bt_matches: output too small')
    v = array.array('I', bytes(buf)[:4 * w])
    out, k = [], 0
    while k < w:
        i, c = v[k], v[k + 1]
        out.append((i, [(v[k + 2 + 2 * q], v[k + 3 + 2 * q]) for q in range(c)]))
        k += 2 + 2 * c
    return out


def peek_size(data):
    return lib().oracle_peek_decoded_size(data, len(data))


def decode(data, out_size=None, dictionary=None):
    """oracle engine brotliDecode: returns bytes, or the negative reference error code (int)."""
    if out_size is None:
        p = peek_size(data)
        out_size = p if p > 0 else -1
    o, n = _P(), ctypes.c_size_t()
    d = bytes(dictionary) if dictionary is not None else None   # an empty dictionary is still attached
    rc = lib().oracle_decode(data, len(data), d, len(d) if d is not None else 0, out_size, ctypes.byref(o),
                             ctypes.byref(n))
    if rc:
        return rc
    r = ctypes.string_at(o, n.value)
    lib().oracle_free(o)
    return r


PROBE_DTYPE = None


def word_refs():
    """static-dictionary word references the oracle decoder has met in this process"""
    lib().oracle_word_refs.restype = ctypes.c_uint64
    return lib().oracle_word_refs()


def compound_refs():
    """compound-dictionary (customDictionary) copies the oracle decoder has met in this process"""
    lib().oracle_compound_refs.restype = ctypes.c_uint64
    return lib().oracle_compound_refs()


def dist_code_counts():
    """copies the oracle decoder has decoded on this thread since the last call, by distance
    code: [implicit (command code < 128), code 0, short codes 1-15, explicit distances]"""
    out = (ctypes.c_uint64 * 4)()
    lib().oracle_dist_code_counts(out)
    return list(out)


def probe(data, positions):
    """decoder states (parts.h PartEntry layout) at the given ascending output positions:
    the command starting there, or the metablock header starting there (flags bit 2)."""
    import numpy as np
    from _parts import ENTRY_DTYPE
    pos = np.ascontiguousarray(np.asarray(positions, dtype=np.uint64))
    out = np.zeros(len(pos), dtype=ENTRY_DTYPE)
    f = lib().oracle_decode_probe
    f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    rc = f(data, len(data), pos.ctypes.data, len(pos), out.ctypes.data)
    if rc:
        raise RuntimeError('oracle_decode_probe rc=%d' % rc)
    return out


class _TraceCode(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('index', ctypes.c_int32), ('alphabet', ctypes.c_int32),
                ('mb', ctypes.c_int32), ('begin', ctypes.c_int64), ('end', ctypes.c_int64),
                ('hist', ctypes.POINTER(ctypes.c_uint32))]


class _TraceMap(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('mb', ctypes.c_int32), ('size', ctypes.c_int32),
                ('ntrees', ctypes.c_int32), ('begin', ctypes.c_int64), ('end', ctypes.c_int64),
                ('values', _P)]


# OracleTraceCode.kind
LITERAL, COMMAND, DISTANCE, BLOCK_TYPE, BLOCK_COUNT, CONTEXT_MAP = 0, 1, 2, 3, 6, 9
KIND_NAMES = {0: 'literal', 1: 'command', 2: 'distance', 3: 'literal block type', 4: 'command block type',
              5: 'distance block type', 6: 'literal block count', 7: 'command block count',
              8: 'distance block count', 9: 'literal context map code', 10: 'distance context map code'}


def trace(data, dictionary=None):
    """decode `data` with the oracle's trace on.  Returns a dict: 'result' (the decoded bytes, or
    the negative error code), 'codes' (every prefix code read: dicts of kind, index, alphabet, mb,
    begin, end, hist -- a list of counts), 'maps' (both context maps of every compressed metablock:
    kind, mb, size, ntrees, begin, end, values) and 'metablocks' (compressed, stored, metadata,
    empty-last)."""
    L = lib()
    L.oracle_trace.argtypes = [ctypes.c_int]
    L.oracle_trace.restype = None
    L.oracle_trace_codes.argtypes = [ctypes.POINTER(ctypes.POINTER(_TraceCode))]
    L.oracle_trace_codes.restype = ctypes.c_size_t
    L.oracle_trace_maps.argtypes = [ctypes.POINTER(ctypes.POINTER(_TraceMap))]
    L.oracle_trace_maps.restype = ctypes.c_size_t
    L.oracle_trace(1)
    try:
        result = decode(data, out_size=-1, dictionary=dictionary)
        pc, pm = ctypes.POINTER(_TraceCode)(), ctypes.POINTER(_TraceMap)()
        codes = []
        for i in range(L.oracle_trace_codes(ctypes.byref(pc))):
            c = pc[i]
            codes.append({'kind': c.kind, 'index': c.index, 'alphabet': c.alphabet, 'mb': c.mb, 'begin': c.begin,
                          'end': c.end, 'hist': c.hist[:c.alphabet]})
        maps = []
        for i in range(L.oracle_trace_maps(ctypes.byref(pm))):
            m = pm[i]
            maps.append({'kind': m.kind, 'mb': m.mb, 'size': m.size, 'ntrees': m.ntrees, 'begin': m.begin,
                         'end': m.end, 'values': list(m.values[:m.size])})
        mbs = (ctypes.c_int32 * 4)()
        L.oracle_trace_metablocks(mbs)
    finally:
        L.oracle_trace(0)
    return {'result': result, 'codes': codes, 'maps': maps, 'metablocks': tuple(mbs)}


def create_huffman_tree(hist, limit=15):
    """the reference's createHuffmanTree: (depths, count limits tried)"""
    n = len(hist)
    h = (ctypes.c_uint32 * n)(*hist)
    d = (ctypes.c_uint8 * n)()
    f = lib().oracle_create_huffman_tree
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    attempts = f(h, n, limit, d)
    return list(d), attempts


def build_store_tree(hist):
    """the reference's buildAndStoreHuffmanTree for one histogram over len(hist) symbols:
    (bytes, bit count, depths, codes)"""
    n = len(hist)
    h = (ctypes.c_uint32 * n)(*hist)
    d = (ctypes.c_uint8 * n)()
    c = (ctypes.c_uint16 * n)()
    cap = 2 * n + 64
    out = (ctypes.c_uint8 * cap)()
    f = lib().oracle_build_store_tree
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    f.restype = ctypes.c_int64
    nbits = f(h, n, d, c, out, cap)
    if nbits < 0:
        raise RuntimeError('oracle_build_store_tree: output too small')
    return bytes(out[:(nbits + 7) // 8]), nbits, list(d), list(c)


def encode_context_map(values, ntrees):
    """the reference's encodeContextMap of a decoded map over ntrees trees: (bytes, bit count)"""
    n = len(values)
    v = (ctypes.c_uint32 * n)(*values)
    cap = 4 * n + 1024
    out = (ctypes.c_uint8 * cap)()
    f = lib().oracle_encode_context_map
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    f.restype = ctypes.c_int64
    nbits = f(v, n, ntrees, out, cap)
    if nbits < 0:
        raise RuntimeError('oracle_encode_context_map: output too small')
    return bytes(out[:(nbits + 7) // 8]), nbits


def max_block_types():
    """the largest (literal, command, distance) block type counts of any metablock the oracle
    decoder has decoded on this thread since the last call"""
    out = (ctypes.c_int * 3)()
    lib().oracle_max_block_types(out)
    return list(out)


def max_table_total():
    """the largest total of one metablock's literal, command and distance tree groups (their
    roots and tables, in entries) the oracle decoder has built on this thread since the last call"""
    lib().oracle_max_table_total.restype = ctypes.c_int
    return lib().oracle_max_table_total()
