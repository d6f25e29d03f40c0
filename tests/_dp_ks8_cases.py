"""The inputs of tests/test_gpu_dp_ks8.py and of scripts/make_dp_ks8_digests.py, which records
the fixture tests/golden/dp_ks8_digests.json: every input is seeded, so the generator and the
test encode the same bytes.  Digests are per stream: its compressed size and SHA-256.

The eight-piece build of the parse (dp_kernel<8>, enc_parse.hip) takes a call's second pass
when it is not FONT mode, has no candidates or custom dictionary, every segment of the call
has at least eight pieces (always, without an experiment's knob) and one encode lane's pieces
number at least THRESHOLD (dp_ks, kKs8Segs).  Pieces per stream (encode.hip dp_piece_shift): a
one-shot stream of one 64 KiB segment has 64 of 1 KiB, a longer one below 1 MiB 32 of 2 KiB a
segment, from 1 MiB on 8 of 8 KiB a segment.  A call splits into two lanes when its streams
span at least 64 MiB of positions (each stream: its segments and one more, 64 KiB each); the
lanes then take near-equal positions, and each lane's parse counts its own pieces.  A single
stream's call (brotliEncode) has at most 2,048 pieces up to 16 MiB: the one-piece build.
"""
import hashlib
import random

import _inputs
import brotli_amd
from brotli_amd import datagen

THRESHOLD = 8704                  # kKs8Segs
MIB = 1 << 20
OPTS = {'quality': 11}

WORDS = (b'international', b'information', b'development', b'environment', b'government', b'understanding',
         b'management', b'experience', b'particular', b'performance', b'available', b'community', b'technology',
         b'everything', b'interesting', b'particularly', b'different', b'important', b'university', b'education')

_cache = {}
_device = {}   # 'mib': the device tensors of its last encode (input, compressed, offsets)


def _text(length, seed):
    return _inputs.resolve({'kind': 'enwik', 'len': length, 'seed': seed})


def _rand(length, seed):
    return _inputs.resolve({'kind': 'xorshift', 'len': length, 'seed': seed})


def _segments(count, seed):
    """count text streams of one 64 KiB segment each: slices of one seeded text"""
    t = _text(count << 16, seed)
    return [t[i << 16:(i + 1) << 16] for i in range(count)]


def _long_run():
    """a 70,000-byte run of one byte from offset 1,000 (the forced long copy and its saturated
    measuring loop; the run crosses the segment end at 65,536, which cuts the copy), then a
    300-byte block repeated (copies of more than 200 bytes at distance 300), text between"""
    blk = _rand(300, 171)
    return _text(1000, 172) + b'\x55' * 70000 + _text(5000, 173) + blk * 200 + _text(3000, 174) + blk * 40


def _words():
    rng = random.Random(15)
    out = bytearray()
    while len(out) < 65536:
        out += rng.choice(WORDS) + rng.choice((b' ', b', ', b'. ', b' the ', b' of '))
    return bytes(out[:65536]) + _text(65536, 190)


# ragged: where each special stream stands among the one-segment text streams
RAGGED_SPECIAL = {
    3: 'seg_plus_1',      # 65,536 + 1 B: a second segment of one byte, 31 of its 32 pieces empty
    20: 'two_segs_tail',  # 131,072 + 3,000 B: a last segment with two pieces of 32 used
    37: 'small',          # 3,000 B: three 1 KiB pieces of 64 used
    38: 'empty',
    39: 'stored',         # 40 B: no segment, no piece
    60: 'random',
    90: 'long_run',
    120: 'words',         # static-dictionary words through its first 64 KiB, 65,536 B of text after
}
# 130 one-segment streams (8,320 pieces) and the special ones' 64 + 96 + 64 + 0 + 0 + 64 + 96 + 64:
# 8,768 pieces in one lane
RAGGED_COUNT = 138


def _ragged():
    fill = iter(_segments(RAGGED_COUNT - len(RAGGED_SPECIAL), 143))
    special = {
        'seg_plus_1': lambda: _text(65537, 161),
        'two_segs_tail': lambda: _text(131072 + 3000, 162),
        'small': lambda: _text(3000, 163),
        'empty': lambda: b'',
        'stored': lambda: _rand(40, 164),
        'random': lambda: _rand(65536, 165),
        'long_run': _long_run,
        'words': _words,
    }
    return [special[RAGGED_SPECIAL[k]]() if k in RAGGED_SPECIAL else next(fill) for k in range(RAGGED_COUNT)]


def pieces(n):
    """parse pieces of a one-shot stream of n bytes (below 64 bytes a stream is stored: it has
    no segment and no piece)"""
    if n < 64:
        return 0
    segs = (n + 65535) >> 16
    return segs * (64 if n <= 65536 else 32 if n < MIB else 8)


def positions(n):
    return (((n + 65535) >> 16) + 1) << 16


MIB_LEN = MIB + 5
# 17 segments of 8 pieces a stream; the call spans more than 64 MiB of positions, so it runs
# as two lanes: the smallest count whose lanes each cross THRESHOLD
MIB_COUNT = 2 * -(-THRESHOLD // pieces(MIB_LEN))


def _build(name):
    if name == 'at_threshold':
        # THRESHOLD / 64 one-segment streams: one lane, exactly THRESHOLD pieces of 1 KiB
        return _segments(THRESHOLD // 64, 141)
    if name == 'below_threshold':
        # the same batch without its last stream: the build the parent took (two pieces a wave)
        return buffers('at_threshold')[:-1]
    if name == 'ragged':
        return _ragged()
    if name == 'two_lanes':
        # 512 one-segment streams: 64 MiB of positions, the smallest batch that splits (the
        # threshold asks for less); lanes of 256 streams, 16,384 pieces each
        return _segments(512, 142)
    raise KeyError(name)


CASES = ('at_threshold', 'below_threshold', 'ragged', 'two_lanes', 'mib')
# the streams that must equal their single-stream encodes (the one-piece build): the first, the
# last, those at a lane cut, the long-run stream and the ragged tails
SOLO = {
    'at_threshold': (0, THRESHOLD // 64 - 1),
    'below_threshold': (0, THRESHOLD // 64 - 2),
    'ragged': (0, RAGGED_COUNT - 1) + tuple(sorted(RAGGED_SPECIAL)),
    'two_lanes': (0, 255, 256, 511),
    'mib': (0, MIB_COUNT // 2 - 1, MIB_COUNT // 2, MIB_COUNT - 1),
}
# the streams the oracle decodes
ORACLE = {
    'at_threshold': (0, 1, 70, THRESHOLD // 64 - 1),
    'below_threshold': (0, THRESHOLD // 64 - 2),
    'ragged': tuple(sorted(RAGGED_SPECIAL)) + (0, RAGGED_COUNT - 1),
    'two_lanes': (0, 255, 256, 511),
    'mib': (0, MIB_COUNT - 1),
}


def buffers(name):
    """the case's inputs as bytes ('mib': generated on the device, copied back)"""
    if name not in _cache:
        if name == 'mib':
            data = _mib_device()
            host = data.cpu().numpy().tobytes()
            _cache[name] = [host[i * MIB_LEN:(i + 1) * MIB_LEN] for i in range(MIB_COUNT)]
        else:
            _cache[name] = _build(name)
    return _cache[name]


def _mib_device():
    import torch
    if 'data' not in _device:
        _device['data'] = datagen.enwik_device(MIB_COUNT * MIB_LEN, 2100, torch.device('cuda', 0))
        # (the context encodes on a stream of its own, which does not wait for torch's: the
        # input must be complete before the call, as bench.py makes sure too)
        torch.cuda.synchronize()
    return _device['data']


def lanes(name):
    """per encode lane of the case's call: its pieces by the rules above (the test holds this
    against the launches the library counts)"""
    sizes = [MIB_LEN] * MIB_COUNT if name == 'mib' else [len(b) for b in buffers(name)]
    total = sum(positions(n) for n in sizes)
    if total < (64 << 20):
        return [sum(pieces(n) for n in sizes)]
    j, pos = 0, 0   # (encode_streams: lane 0 takes streams until half the positions)
    while j < len(sizes) - 1 and (j == 0 or pos * 2 < total):
        pos += positions(sizes[j])
        j += 1
    return [sum(pieces(n) for n in sizes[:j]), sum(pieces(n) for n in sizes[j:])]


def encode(name):
    """the case's streams from the loaded library"""
    if name != 'mib':
        return brotli_amd.encode_batch(buffers(name), OPTS)
    import torch
    data = _mib_device()
    k, n = MIB_COUNT, MIB_LEN
    cap = k * n + k * n // 8 + 4096 * k
    comp = torch.empty(cap, dtype=torch.uint8, device=data.device)
    ctx = brotli_amd.DeviceContext(0)
    off = ctx.encode(data.data_ptr(), [i * n for i in range(k + 1)], comp.data_ptr(), cap, OPTS)
    _device.update(comp=comp, off=off, ctx=ctx)
    raw = comp[:off[-1]].cpu().numpy().tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(k)]


def mib_device_roundtrip():
    """decode the last 'mib' encode on the device and compare there; True when every stream
    came back as its input"""
    import torch
    data, comp, off, ctx = _device['data'], _device['comp'], _device['off'], _device['ctx']
    k, n = MIB_COUNT, MIB_LEN
    slot = n + 4096 - n % 4096 + 4096
    out = torch.empty(k * slot, dtype=torch.uint8, device=data.device)
    sizes, status = ctx.decode(comp.data_ptr(), off, out.data_ptr(), [i * slot for i in range(k + 1)])
    return status == [0] * k and sizes == [n] * k and bool(torch.equal(out.view(k, slot)[:, :n], data.view(k, n)))


def digest(streams):
    return [[len(s), hashlib.sha256(s).hexdigest()] for s in streams]
