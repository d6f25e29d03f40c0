"""The inputs of tests/test_gpu_backtrack.py and of scripts/make_backtrack_digests.py, which
records the fixture tests/golden/backtrack_digests.json: every input is seeded, so the generator
and the test encode the same bytes.  Digests are per stream: its compressed size and SHA-256.

backtrack_kernel (enc_parse.hip) walks a segment's (or a parse piece's) path from its end in
windows of 64 positions aligned to that end, four windows (a chunk of 256 positions) loaded at
a time.  The cases are the smallest shapes at which that walk can go wrong: segments shorter
than a window or a chunk, windows without a copy, copies that end or start on a window or a
chunk edge, a forced long copy that jumps past the next chunk, dense short copies, 2 KiB and
8 KiB pieces -- and calls that find the previous call's choices under every position, the
interiors of long copies included, since nothing zeroes them.
"""
import hashlib

import _dp_ks8_cases as ks8
import _inputs
import brotli_amd

MIB = 1 << 20
FONT = brotli_amd.EncoderMode.FONT


def _text(length, seed):
    return _inputs.resolve({'kind': 'enwik', 'len': length, 'seed': seed})


def _rand(length, seed):
    return _inputs.resolve({'kind': 'xorshift', 'len': length, 'seed': seed})


SHORT = (64, 65, 127, 128, 129, 255, 256, 257, 3000)
EDGE = (64, 63, 65, 128, 256, 257)

_cache = {}


def _edge(n):
    """X = n random bytes, 500 other random bytes, X again at the stream's end: the last command
    is a copy of n bytes ending at the segment end, where the windows are aligned"""
    x = _rand(n, 300 + n)
    return x + _rand(500, 700 + n) + x


def _build(name):
    if name == 'short_text':
        return [_text(n, 200 + n) for n in SHORT]
    if name == 'random':
        return [_rand(3000, 251)]
    if name == 'edge_copies':
        return [_edge(n) for n in EDGE]
    if name == 'long_run':
        return [ks8._long_run()]
    if name == 'long_run_twin':
        # text of the long-run stream's length: the same workspace, other choices (stale_choices)
        return [_text(len(buffers('long_run')[0]), 252)]
    if name == 'text_64k':
        return [_text(65536, 253)]
    if name == 'two_segs_tail':
        return [_text(131072 + 3000, 254)]   # 2 KiB pieces; a last segment of 3,000 bytes
    if name == 'mib':
        return [_text(MIB + 5, 255)]         # 8 KiB pieces; a last segment of 5 bytes
    if name == 'two_lanes':
        return ks8._segments(512, 142)       # 64 MiB of positions: two encode lanes of 256 streams
    if name == 'mixed':
        # one call over every shape above: pieces of 1, 2 and 8 KiB in one launch
        return [b for n in SOLO_CASES for b in buffers(n)]
    raise KeyError(name)


def buffers(name):
    name = name.split('@')[0]
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


# every stream of these is encoded by a call of its own (brotliEncode), quality 11
SOLO_CASES = ('short_text', 'random', 'edge_copies', 'long_run', 'long_run_twin', 'text_64k', 'two_segs_tail', 'mib')
# one encode_batch call each.  Every stream of 'mixed' must equal its solo encode, and so must the
# streams of 'two_lanes' at the lane cut; 'two_lanes' has no digests of its own (its 512 streams are
# those of tests/_dp_ks8_cases.py's case of that name, recorded there)
BATCH_CASES = ('mixed', 'two_lanes')
TWO_LANES_SOLO = (0, 255, 256, 511)
# four of the inputs again at other qualities and in FONT mode, solo
OTHER = ('edge_copies', 'long_run', 'text_64k', 'two_segs_tail')
VARIANTS = {'q5': {'quality': 5}, 'q9': {'quality': 9}, 'q10': {'quality': 10}, 'font': {'quality': 11, 'mode': FONT}}
OTHER_CASES = tuple('%s@%s' % (n, v) for n in OTHER for v in VARIANTS)
CASES = SOLO_CASES + ('mixed',) + OTHER_CASES   # the cases with recorded digests
# the streams the oracle decodes
ORACLE = {'short_text': (0, 1, 8), 'edge_copies': (0, 3), 'long_run': (0,), 'mib': (0,),
          'long_run@q5': (0,), 'text_64k@font': (0,)}


def options(name):
    return VARIANTS[name.split('@')[1]] if '@' in name else {'quality': 11}


def encode(name):
    """the case's streams from the loaded library"""
    if name in BATCH_CASES:
        return brotli_amd.encode_batch(buffers(name), options(name))
    return [brotli_amd.brotliEncode(b, options(name)) for b in buffers(name)]


def stale_choices():
    """One DeviceContext, so one workspace: the batch of both streams first (the workspace then
    has its largest size and is not allocated again), then the long-run stream, the text of its
    length, the long-run stream again and the batch again.  Each call finds the choices of the
    call before under every position it parses.  Returns the five calls' streams."""
    import torch
    dev = torch.device('cuda', 0)
    a, b = buffers('long_run')[0], buffers('long_run_twin')[0]
    n = len(a)
    data = torch.frombuffer(bytearray(a + b), dtype=torch.uint8).to(dev)
    cap = 2 * n + n // 4 + 8192
    comp = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx = brotli_amd.DeviceContext(0)
    out = []
    for offs in ([0, n, 2 * n], [0, n], [n, 2 * n], [0, n], [0, n, 2 * n]):
        off = ctx.encode(data.data_ptr(), offs, comp.data_ptr(), cap, {'quality': 11})
        raw = comp[:off[-1]].cpu().numpy().tobytes()
        out.append([raw[off[i]:off[i + 1]] for i in range(len(offs) - 1)])
    ctx.close()
    return out


def digest(streams):
    return [[len(s), hashlib.sha256(s).hexdigest()] for s in streams]
