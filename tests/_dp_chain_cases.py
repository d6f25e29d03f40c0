"""The inputs of tests/test_gpu_dp_chain.py and of scripts/make_dp_chain_digests.py, which
records the fixture tests/golden/dp_chain_digests.json: every input is seeded
(brotli_amd.datagen, tests/_inputs.py), so the generator and the test encode the same bytes.

A case is (name, buffers, how): `how` says which call encodes the buffers.  Every case's
digests are per stream: sha256 of the stream's bytes and its compressed size.

The parse's builds by the numbers of encode.hip / enc_parse.hip: a one-shot stream of at most
one 64 KiB segment is cut into 64 parse pieces of 1 KiB, a longer one below 1 MiB into 2 KiB
pieces, from 1 MiB on into 8 KiB pieces (dp_piece_shift).  dp_ks() takes the four-segment
build from 12,288 pieces on, the one-segment build up to 2,048, the two-segment build
between; FONT mode stays at two.  A call splits into two encode lanes when its streams span
at least 64 MiB of positions (each stream: its segments and one more, 64 KiB each), and each
lane's parse counts its own pieces.  q11 parses twice: the first pass over whole segments
(here always the one-segment build, KM off), the second over the pieces (KM on).
"""
import hashlib
import random

import _inputs
import brotli_amd
from brotli_amd import datagen

FONT = brotli_amd.EncoderMode.FONT
GENERIC = brotli_amd.EncoderMode.GENERIC

EDGE_SIZES = (1, 2, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 65535, 65536, 65537, 131073)
PERIODS = (1, 3, 17, 200, 201, 1000)

WORDS = (b'international', b'information', b'development', b'environment', b'government', b'understanding',
         b'management', b'experience', b'particular', b'performance', b'available', b'community', b'technology',
         b'everything', b'interesting', b'particularly', b'different', b'important', b'university', b'education')

_cache = {}


def _text(length, seed):
    return _inputs.resolve({'kind': 'enwik', 'len': length, 'seed': seed})


def _rand(length, seed):
    return _inputs.resolve({'kind': 'xorshift', 'len': length, 'seed': seed})


def _segments(count, seed):
    """count text streams of one 64 KiB segment each: slices of one seeded text"""
    t = _text(count << 16, seed)
    return [t[i << 16:(i + 1) << 16] for i in range(count)]


def records(n, seed, rec=48):
    """binary records, each the one one or two records back with a few bytes changed"""
    rng = random.Random(seed)
    out = bytearray(rng.getrandbits(8) for _ in range(2 * rec))
    while len(out) < n:
        back = rec if rng.random() < 0.7 else 2 * rec
        r = bytearray(out[len(out) - back:len(out) - back + rec])
        for _ in range(rng.randrange(1, 4)):
            r[rng.randrange(rec)] = rng.getrandbits(8)
        out += r
    return bytes(out[:n])


def _build(name):
    if name == 'ks4':
        # 512 x 65,536 B: 64 MiB of positions, two lanes of 256 streams; each lane 256 x 64 =
        # 16,384 pieces (>= 12,288: the four-segment build); its first pass 256 segments (one)
        return _segments(512, 41)
    if name == 'ks2':
        # 64 x 65,536 B: one lane, 64 x 64 = 4,096 pieces (2,048 < n < 12,288: two segments)
        return _segments(64, 42)
    if name == 'ks1':
        # 16 x 65,536 B: one lane, 1,024 pieces (<= 2,048: one segment)
        return _segments(16, 43)
    if name == 'edges':
        return [_text(n, 50 + k) for k, n in enumerate(EDGE_SIZES)]
    if name == 'periodic':
        # a one-byte run and periods 3 .. 1,000, 256 KiB each: saturated matches (255+), long
        # copies (> 200) that restart a batch mid-wave, staircases over many chunks
        return [(_rand(p, 60 + p) * (262144 // p + 1))[:262144] for p in PERIODS]
    if name == 'random':
        return [_rand(131072, 71)]
    if name == 'mixed':
        # 35 x 128 KiB, random and text by turns, and a 3,000-byte tail: 35 x 64 pieces of 2 KiB
        # and the tail's 64 of 1 KiB (most of them empty: idle lane groups) = 2,304 pieces, the
        # two-segment build with neighbouring streams' pieces in one wave
        return [_rand(131072, 80 + k) if k % 2 == 0 else _text(131072, 80 + k) for k in range(35)] + [_text(3000, 79)]
    if name == 'words':
        # static-dictionary words (a word's copy has minlen = its length) through the first 64 KiB
        rng = random.Random(5)
        out = bytearray()
        while len(out) < 65536:
            out += rng.choice(WORDS) + rng.choice((b' ', b', ', b'. ', b' the ', b' of '))
        return [bytes(out[:65536]) + _text(65536, 90)]
    if name == 'font':
        return [_inputs.resolve({'kind': 'glyf', 'len': 262144, 'seed': 1007})]
    if name == 'records':
        return [records(200000, 7)]
    if name == 'cdict':
        d = datagen.c5_dictionary()
        return [d[-150:] + _text((3 << 20) - 150, 31)]
    raise KeyError(name)


# name -> (options, how): 'batch' = encode_batch, 'stream' = BrotliEncoder in 1 MiB chunks
CASES = {
    'ks4': ({'quality': 11}, 'batch'),
    'ks2': ({'quality': 11}, 'batch'),
    'ks1': ({'quality': 11}, 'batch'),
    'edges': ({'quality': 11}, 'batch'),
    'periodic': ({'quality': 11}, 'batch'),
    'random': ({'quality': 11}, 'batch'),
    'mixed': ({'quality': 11}, 'batch'),
    'words': ({'quality': 11}, 'batch'),
    'font': ({'quality': 11, 'mode': FONT}, 'batch'),
    'records': ({'quality': 11, 'mode': GENERIC}, 'batch'),
    'cdict': ({'quality': 11}, 'stream'),
}
# the streams of ks4 that must also equal their single-stream encodes: the first, the last and
# the two at the lane boundary
KS4_SOLO = (0, 255, 256, 511)


def buffers(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def options(name):
    o = dict(CASES[name][0])
    if name == 'cdict':
        o['customDictionary'] = datagen.c5_dictionary()
    return o


def encode(name):
    """the case's streams from the loaded library"""
    bufs, o = buffers(name), options(name)
    if CASES[name][1] == 'batch':
        return brotli_amd.encode_batch(bufs, o)
    enc = brotli_amd.BrotliEncoder(o)
    data = bufs[0]
    parts = [enc.update(data[i:i + (1 << 20)]) for i in range(0, len(data), 1 << 20)]
    parts.append(enc.finish())
    return [b''.join(parts)]


def digest(streams):
    return [[len(s), hashlib.sha256(s).hexdigest()] for s in streams]
