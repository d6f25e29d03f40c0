"""A prepared dictionary (brotli_amd.Dictionary; mib_dictionary in brotli_amd.h) on the GPU.

The decoder first: hand-written streams whose compound copies sit at every placement the standard
rule distinguishes, expectations from tests/_shared_dict.py (never from the engine).  Then the
encoder, by round trips through the decoder just pinned; that the dictionary is used; batches and
threads; the Python mirror."""
import base64
import json
import os
import random
import shutil
import subprocess
import threading

import pytest

import brotli_amd
from brotli_amd import BrotliError, Dictionary, EncoderMode

import _shared_dict as sd

pytestmark = pytest.mark.gpu

CASES = sd.decoder_cases()
MID = [c for c in CASES if c[0] == 'middle'][0]


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


DICT64K = _rand(1234, 65536)


@pytest.fixture(scope='module')
def small():
    with Dictionary(sd.DICT) as d:
        yield d


@pytest.fixture(scope='module')
def big():
    with Dictionary(DICT64K) as d:
        yield d


def _decode(streams, d, **kw):
    return brotli_amd.decode_batch(streams, dictionary=d, **kw)


def _code(r):
    return r.code if isinstance(r, BrotliError) else None


# ---------------------------------------------------------------- decoder
@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_decoder_placements(small, name):
    _, stream, dic = [c for c in CASES if c[0] == name][0]
    want, err = sd.model(stream, dic)
    got = _decode([sd.build(stream, dic).data], small)[0]
    if err is None:
        assert got == want
    else:
        assert _code(got) == err
    # k = 1 through brotliDecode
    if err is None:
        assert brotli_amd.brotliDecode(sd.build(stream, dic).data, {'dictionary': small}) == want
    else:
        with pytest.raises(BrotliError) as e:
            brotli_amd.brotliDecode(sd.build(stream, dic).data, {'dictionary': small})
        assert e.value.code == err


def test_decoder_slots_are_independent(small):
    """the same stream twice, beside a corrupt stream, an empty input and a copy past the end"""
    good = sd.build(MID[1], sd.DICT).data
    want = sd.model(MID[1], sd.DICT)[0]
    bad = [c for c in CASES if c[0] == 'one_past_the_end'][0]
    corrupt = bytes([good[0]]) + bytes(b ^ 0xFF for b in good[1:])
    alone = [_decode([s], small)[0] for s in (corrupt, b'')]
    res = _decode([good, corrupt, b'', good, sd.build(bad[1], sd.DICT).data], small)
    assert res[0] == want and res[3] == want
    assert _code(res[1]) is not None and _code(res[1]) == _code(alone[0])
    assert _code(res[2]) is not None and _code(res[2]) == _code(alone[1])
    assert _code(res[4]) == -9


def test_max_out_trips_one_slot(small):
    whole = [c for c in CASES if c[0] == 'whole_dictionary'][0]
    short, long_ = sd.build(MID[1], sd.DICT).data, sd.build(whole[1], sd.DICT).data
    res = _decode([short, long_, short], small, options={'maxOutputSize': 50})
    want = sd.model(MID[1], sd.DICT)[0]
    assert res[0] == want and res[2] == want
    assert _code(res[1]) == -103 and '100' in str(res[1])
    assert _decode([long_], small, options={'maxOutputSize': 100})[0] == sd.model(whole[1], sd.DICT)[0]


def test_reference_rule_is_unchanged_and_its_streams_are_read(small):
    mid = sd.build(MID[1], sd.DICT).data
    with pytest.raises(BrotliError) as e:
        brotli_amd.brotliDecode(mid, {'customDictionary': sd.DICT})
    assert e.value.code == -9
    # a stream of the customDictionary encoder (tail copies only) is valid under the standard rule
    with Dictionary(DICT64K[:8192]) as d:
        # (340 bytes, 240 of them two tails of the dictionary: that encoder copies tails of up to
        # 200 bytes, so the stream is little more than the 100 bytes of noise)
        data = DICT64K[8192 - 150:8192] + _rand(5, 100) + DICT64K[8192 - 90:8192]
        enc = brotli_amd.brotliEncode(data, {'quality': 9, 'customDictionary': DICT64K[:8192]})
        assert len(enc) < 170
        assert _decode([enc], d)[0] == data


# ---------------------------------------------------------------- encoder: round trips
def _documents(D, lgwin):
    """documents built from slices of D (names for the failure message)"""
    r = random.Random(77)
    n = len(D)

    def noise(k):
        return r.randbytes(k)

    def cut(k):
        a = r.randrange(0, n - k)
        return D[a:a + k]
    docs = [
        ('address_0', D[:300] + noise(80)),
        ('last_byte_then_zeros', noise(70) + D[-500:] + bytes(64)),
        ('straddles_64k', noise(65536 - 100) + D[1000:1200] + noise(40)),
        ('last_4_bytes', noise(100) + D[5000:5104]),
        ('600_bytes', noise(50) + D[2000:2600] + noise(50)),
        ('non_utf8_between', b''.join(cut(r.randrange(20, 120)) + bytes(r.randrange(128, 256) for _ in range(r.randrange(1, 9)))
                                      for _ in range(40))),
        ('one_byte_changed', b''.join(D[3000 + 50 * i:3050 + 50 * i] + b'\xfe' for i in range(30))),
        ('empty', b''), ('1', D[7:8]), ('63', D[100:163]), ('64', D[100:164]),
        ('4k_of_slices', b''.join(cut(256) for _ in range(16))),
    ]
    # a slice ending on an 8 KiB piece boundary B, then a window copy of the same distance: at B the
    # stream's first bytes lie B back, and the slice (from address n - L at B - L) has distance B too
    for B in (8192, 16384):
        L = 37
        head = noise(B - L)
        docs.append(('piece_boundary_%d' % B, head + D[-L:] + head[:300] + noise(500)))
        a = 4000
        head = noise(B - L)
        # (the same with a slice from the middle: its distance at B - L is B - L + n - a; the window
        # copy behind it repeats what lies that far back only if the document is that long)
        docs.append(('piece_boundary_mid_%d' % B, head + D[a:a + L] + head[:200] + noise(100)))
    return docs


@pytest.mark.parametrize('mode', [EncoderMode.GENERIC, EncoderMode.FONT])
@pytest.mark.parametrize('lgwin', [10, 16, 22, 24])
@pytest.mark.parametrize('q', [1, 5, 9, 11])
def test_round_trip_grid(big, q, lgwin, mode):
    docs = _documents(DICT64K, lgwin)
    enc = brotli_amd.encode_batch([d for _, d in docs], {'quality': q, 'lgwin': lgwin, 'mode': mode}, dictionary=big)
    dec = _decode(enc, big)
    for (name, d), e, got in zip(docs, enc, dec):
        assert got == d, (name, q, lgwin, mode, got if isinstance(got, BrotliError) else 'bytes differ')
    # the slices are found: the slice documents shrink (noise does not compress)
    by = {name: len(e) for (name, _), e in zip(docs, enc)}
    if q >= 5:
        assert by['600_bytes'] < 200
        assert by['4k_of_slices'] < 1024


@pytest.mark.parametrize('n', [0, 3, 4])
def test_tiny_dictionaries(n):
    with Dictionary(DICT64K[:n]) as d:
        assert len(d) == n
        docs = [DICT64K[:n] * 40, b'hello hello hello hello hello hello hello hello hello hello hello hello the and of', b'']
        for q in (5, 11):
            enc = brotli_amd.encode_batch(docs, {'quality': q}, dictionary=d)
            assert _decode(enc, d) == docs


def test_dictionary_longer_than_the_match_span():
    """lgwin 16: the span is 0xFFFFFE - (2^16 - 16) bytes; the dictionary is 4 KiB longer.  Beyond
    max backward a slice in front of the span round-trips as literals and one inside it is copied.
    (At the stream's start the front slice's distance would fit a record, but the index keeps each
    bucket's eight highest addresses, which in 16 MiB of noise lie in its last MiB or so: that
    document only has to round-trip.)"""
    span = 0xFFFFFE - ((1 << 16) - 16)
    D = _rand(9, span + 4096)
    far = _rand(4, 70000)   # (past max backward = 65,520: the distance is 65,520 + dictionary size - address)
    with Dictionary(D) as d:
        assert len(d) == len(D)
        docs = [far + D[100:600] + _rand(1, 20), far + D[-3000:-2500] + _rand(2, 20), D[100:600] + _rand(3, 20)]
        enc = brotli_amd.encode_batch(docs, {'quality': 5, 'lgwin': 16}, dictionary=d)
        assert _decode(enc, d) == docs
        # (noise does not compress: a document shrinks by what its 500-byte slice saves)
        assert len(enc[0]) > len(docs[0]) - 100 and len(enc[1]) < len(docs[1]) - 300


def test_two_mib_stream_takes_the_part_parallel_path(big):
    r = random.Random(3)
    n = (2 << 20) + 1
    parts, size = [], 0
    while size < n:
        k = r.randrange(200, 3000)
        a = r.randrange(0, len(DICT64K) - k)
        parts.append(DICT64K[a:a + k] + r.randbytes(r.randrange(0, 40)))
        size += len(parts[-1])
    data = b''.join(parts)[:n]
    enc = brotli_amd.encode_batch([data], {'quality': 5}, dictionary=big)[0]
    assert len(enc) < n // 4
    used0, fell0 = brotli_amd.part_stats()
    assert _decode([enc], big)[0] == data
    used1, fell1 = brotli_amd.part_stats()
    assert used1 == used0 + 1 and fell1 == fell0, 'the stream did not decode part-parallel, or a part did not check out'


# ---------------------------------------------------------------- that the dictionary is used
def _slice_doc(seed):
    r = random.Random(seed)
    return b''.join(DICT64K[a:a + 256] for a in (r.randrange(1000, 60000) for _ in range(16)))


def test_the_dictionary_is_used(big):
    docs = [_slice_doc(s) for s in range(8)]
    for q in (5, 11):
        enc = brotli_amd.encode_batch(docs, {'quality': q}, dictionary=big)
        assert _decode(enc, big) == docs
        old = brotli_amd.encode_batch(docs, {'quality': q, 'customDictionary': DICT64K})
        for d, e, o in zip(docs, enc, old):
            assert len(e) < len(d) // 4, (q, len(e))
            assert len(o) > 0.9 * len(d), (q, len(o))


# ---------------------------------------------------------------- batches and threads
def test_batch_equals_solo_and_the_handle_is_shared(big):
    docs = [_slice_doc(100 + s)[:r] for s, r in zip(range(64), [4096, 4000, 63, 64, 1000, 0, 1, 2500] * 8)]
    opts = {'quality': 9}
    enc = brotli_amd.encode_batch(docs, opts, dictionary=big)
    assert enc == brotli_amd.encode_batch(docs, opts, dictionary=big)   # the handle again
    for i in range(64):
        assert enc[i] == brotli_amd.encode_batch([docs[i]], opts, dictionary=big)[0], i
    assert enc[0] == brotli_amd.brotliEncode(docs[0], dict(opts, dictionary=big))
    assert _decode(enc, big) == docs
    # an encode and a decode call from two threads on the one handle
    out = {}

    def enc_t():
        out['e'] = [brotli_amd.encode_batch(docs, opts, dictionary=big) for _ in range(3)]

    def dec_t():
        out['d'] = [_decode(enc, big) for _ in range(3)]
    ts = [threading.Thread(target=enc_t), threading.Thread(target=dec_t)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(e == enc for e in out['e']) and all(d == docs for d in out['d'])


# ---------------------------------------------------------------- the Python mirror
def test_python_dictionary_lifecycle():
    d = Dictionary(bytearray(DICT64K[:1000]))
    assert len(d) == 1000 and not d.closed
    doc = DICT64K[100:400]
    enc = brotli_amd.brotliEncode(doc, {'dictionary': d})
    assert len(enc) < 40 and brotli_amd.brotliDecode(enc, {'dictionary': d}) == doc
    with pytest.raises(ValueError):
        brotli_amd.brotliEncode(doc, {'dictionary': d, 'customDictionary': b'abcd'})
    with pytest.raises(ValueError):
        brotli_amd.brotliDecode(enc, {'dictionary': d, 'customDictionary': b'abcd'})
    with pytest.raises(TypeError):
        brotli_amd.encode_batch([doc], dictionary=b'not a handle')
    assert brotli_amd.encode_batch([], dictionary=d) == [] and brotli_amd.decode_batch([], dictionary=d) == []
    d.close()
    d.close()
    assert d.closed and len(d) == 1000
    with pytest.raises(ValueError):
        brotli_amd.brotliEncode(doc, {'dictionary': d})
    with Dictionary(b'') as e:
        assert len(e) == 0
        assert brotli_amd.brotliDecode(brotli_amd.brotliEncode(doc, {'dictionary': e}), {'dictionary': e}) == doc
    assert e.closed


# ---------------------------------------------------------------- the Node mirror
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _node_fixture(tmp_path, big):
    """what the Node tests read: the dictionary, documents, the streams the Python mirror wrote
    for them with the handle, and hand-written streams from _shared_dict"""
    def b64(x):
        return base64.b64encode(x).decode()
    docs = [_slice_doc(500 + s)[:n] for s, n in enumerate((4096, 1000, 64, 63, 1, 0, 2500, 300))]
    past = [c for c in CASES if c[0] == 'one_past_the_end'][0]
    fx = {'dictionary': b64(DICT64K), 'quality': 9, 'docs': [b64(d) for d in docs],
          'streams': [b64(e) for e in brotli_amd.encode_batch(docs, {'quality': 9}, dictionary=big)],
          'mid_dictionary': b64(sd.DICT), 'mid_stream': b64(sd.build(MID[1], sd.DICT).data),
          'mid_output': b64(sd.model(MID[1], sd.DICT)[0]), 'past_stream': b64(sd.build(past[1], sd.DICT).data)}
    path = str(tmp_path / 'dictionary_fixture.json')
    with open(path, 'w') as f:
        json.dump(fx, f)
    return path


def _run_node(script, fixture):
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', script), fixture], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout


def test_node_dictionary_mirror(tmp_path, big):
    assert 'ALL OK' in _run_node('dictionary_test.js', _node_fixture(tmp_path, big))


def test_node_zlib_cross_decodes_where_it_takes_a_dictionary(tmp_path, big):
    """the only interoperability evidence to be had: node's zlib is google/brotli's library"""
    out = _run_node('dictionary_zlib_test.js', _node_fixture(tmp_path, big))
    if out.startswith('SKIP'):
        pytest.skip(out.strip())
    assert 'ALL OK' in out
