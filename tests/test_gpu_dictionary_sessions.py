"""BrotliEncoder / BrotliDecoder sessions with a prepared dictionary (options['dictionary'], a
brotli_amd.Dictionary; mib_encoder_new_dictionary / mib_decoder_new_dictionary in brotli_amd.h).

The decoder first: the hand-written streams of tests/_shared_dict.py through sessions, fed whole
and cut in two at many positions, the expectations from that file's model (never from the engine);
a stream that takes several passes, so that the history has moved before its dictionary copies; a
batch of sessions that hold different dictionaries.  Then the encoder, by round trips through the
one-shot decoder and the decoder session just pinned; that the dictionary is used in a chunk that
is not the first; a batch of encoders with a dictionary each; the handle's lifetime; Node."""
import base64
import json
import os
import random
import shutil
import subprocess

import pytest

import brotli_amd
from brotli_amd import BrotliDecoder, BrotliEncoder, BrotliError, Dictionary, EncoderMode

import _shared_dict as sd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sd.decoder_cases()
WIN = 65536          # outWindow of the decoder sessions here (the smallest)
MAX_SESSIONS = 96    # a batch: a session's buffer is 16 MiB of slack plus its windows


def _case(name):
    return [c for c in CASES if c[0] == name][0]


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


DICT64K = _rand(1234, 65536)
_built = {}


def _stream(name):
    """(stream bytes, model output, model error) of a decoder case, built once"""
    if name not in _built:
        _, st, dic = _case(name)
        want, err = sd.model(st, dic)
        _built[name] = (sd.build(st, dic).data, want, err)
    return _built[name]


@pytest.fixture(scope='module')
def small():
    with Dictionary(sd.DICT) as d:
        yield d


@pytest.fixture(scope='module')
def big():
    with Dictionary(DICT64K) as d:
        yield d


def _code(r):
    return r.code if isinstance(r, BrotliError) else None


# ---------------------------------------------------------------- decoder: placements
def _cuts(n):
    """where a stream of n bytes is cut in two: every position of a stream of up to 96 bytes, else
    the first 16, the last 16 and 64 spread evenly between them"""
    if n <= 96:
        return list(range(1, n))
    return sorted(set(list(range(1, 17)) + list(range(n - 16, n)) + [17 + (n - 33) * i // 64 for i in range(64)]))


def _placements(small, name):
    data, want, err = _stream(name)
    cuts = _cuts(len(data))
    assert 0 < len(cuts) <= MAX_SESSIONS
    # fed whole
    whole = _alone({'dictionary': small, 'outWindow': WIN}, data)
    assert (whole == want) if err is None else (_code(whole) == err), name
    # cut in two: the sessions advance together, three launches a case
    ds = [BrotliDecoder({'dictionary': small, 'outWindow': WIN}) for _ in cuts]
    heads = brotli_amd.decoder_update_batch(ds, [data[:c] for c in cuts])
    tails = brotli_amd.decoder_update_batch(ds, [data[c:] for c in cuts])
    fins = brotli_amd.decoder_finish_batch(ds)
    for c, h, t, f in zip(cuts, heads, tails, fins):
        steps = [h, t, f]
        if err is None:
            assert all(isinstance(x, bytes) for x in steps), (name, c, [_code(x) for x in steps])
            assert b''.join(steps) == want, (name, c)
            continue
        # the slot that receives the failing copy carries the error, and every later call repeats it
        codes = [_code(x) for x in steps]
        first = [i for i, x in enumerate(codes) if x is not None]
        assert first, (name, c, 'no error')
        k = first[0]
        assert codes[k:] == [err] * (3 - k), (name, c, codes)
        got = b''.join(steps[:k])
        assert want.startswith(got), (name, c)
    if err is not None:
        again = brotli_amd.decoder_update_batch(ds, [b''] * len(ds))
        assert [_code(x) for x in again] == [err] * len(ds), name
    else:
        assert all(d.finished for d in ds), name


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_decoder_placements(small, name):
    _placements(small, name)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_decoder_placements_four_per_cu_build(small, name):
    """the same batch through the other build of decode_resume_kernel"""
    lib = brotli_amd._L()
    lib.mib_force_decoder_build(1)
    try:
        _placements(small, name)
    finally:
        lib.mib_force_decoder_build(0)


# ---------------------------------------------------------------- decoder: several passes
def _long_stream():
    """lgwin 16: about 200 KB of literals in commands of 1,000 bytes (each ends in a short window
    copy, so a pass has boundaries to stop at), then copies from the dictionary far beyond max
    backward -- 9 bytes from address 0, a code-0 copy (the window term is constant there, so the
    same distance is the same address again), one from the middle, one that ends on the
    dictionary's last byte -- then literals"""
    if 'long' not in _built:
        L = len(sd.DICT)
        r = random.Random(41)
        cmds, pos = [], [0]

        def add(ins, n, spec):
            """spec: None, a spec, or a dictionary address for the copy's position"""
            pos[0] += len(ins)
            if isinstance(spec, int):
                spec = ('dist', sd.distance_of(pos[0], 16, L, spec))
            cmds.append((ins, n, spec))
            pos[0] += n if spec is not None else 0
        for _ in range(200):
            add(r.randbytes(1000), 4, ('dist', 7))
        at = pos[0]
        add(b'', 9, 0)
        add(b'', 6, ('short', 0))
        add(b'xy', 10, 40)
        add(b'z', 6, L - 6)
        add(r.randbytes(300), 2, None)
        st = sd.one(16, cmds, 'long')
        want, err = sd.model(st, sd.DICT)
        assert err is None and len(want) == pos[0] and at == 200 * 1004
        # the copies are what they are meant to be
        assert want[at:at + 34] == sd.DICT[:9] + sd.DICT[:6] + b'xy' + sd.DICT[40:50] + b'z' + sd.DICT[L - 6:]
        _built['long'] = (sd.build(st, sd.DICT).data, want)
    return _built['long']


def test_decoder_several_passes(small):
    data, want = _long_stream()
    dec = BrotliDecoder({'dictionary': small, 'outWindow': WIN})
    out = [dec.update(data[at:at + 50000]) for at in range(0, len(data), 50000)]
    out.append(dec.finish())
    assert b''.join(out) == want
    assert dec.finished
    # (200 KB of output through a 64 KiB window at lgwin 16: the history moved before the copies)
    assert dec.passes > 1
    # and the one-shot decoder agrees about the stream
    assert brotli_amd.decode_batch([data], dictionary=small)[0] == want


# ---------------------------------------------------------------- decoder: a mixed batch
def _mixed_sessions(small, other):
    tail_doc = DICT64K[8192 - 150:8192] + _rand(5, 100) + DICT64K[8192 - 90:8192]
    tail_stream = brotli_amd.brotliEncode(tail_doc, {'quality': 9, 'customDictionary': DICT64K[:8192]})
    plain_doc = b'no dictionary at all, ' * 40
    plain_stream = brotli_amd.brotliEncode(plain_doc, {'quality': 5})
    # the second handle holds other bytes of the same length: the same stream decodes to those
    _, st, _ = _case('middle')
    items = [
        ({'dictionary': small, 'outWindow': WIN}, _stream('middle')[0], sd.model(st, sd.DICT)),
        ({'dictionary': other, 'outWindow': WIN}, sd.build(st, OTHER).data, sd.model(st, OTHER)),
        ({'customDictionary': DICT64K[:8192], 'outWindow': WIN}, tail_stream, (tail_doc, None)),
        ({'outWindow': WIN}, plain_stream, (plain_doc, None)),
        ({'dictionary': small, 'outWindow': WIN}, _stream('one_past_the_end')[0], sd.model(_case('one_past_the_end')[1], sd.DICT)),
    ]
    return items


OTHER = bytes(255 - b for b in sd.DICT)


def _alone(opts, data):
    d = BrotliDecoder(opts)
    try:
        return d.update(data) + d.finish()
    except BrotliError as e:
        return e


def test_decoder_mixed_batch(small):
    with Dictionary(OTHER) as other:
        items = _mixed_sessions(small, other)
        ds = [BrotliDecoder(o) for o, _, _ in items]
        got = brotli_amd.decoder_update_batch(ds, [s for _, s, _ in items])
        fin = brotli_amd.decoder_finish_batch(ds)
        for i, (opts, data, (want, err)) in enumerate(items):
            # what the session gives alone, step by step (an error: its code)
            alone = []
            d = BrotliDecoder(opts)
            for step in (lambda: d.update(data), d.finish):
                try:
                    alone.append(step())
                except BrotliError as e:
                    alone.append(e.code)
            assert [_code(x) if isinstance(x, BrotliError) else x for x in (got[i], fin[i])] == alone, i
            if err is None:
                assert got[i] + fin[i] == want, i
            else:   # (a stream that ends inside the reader's window may be told so only by finish())
                assert _code(fin[i]) == err and (_code(got[i]) == err or want.startswith(got[i])), i
        assert items[0][2][0] != items[1][2][0]   # (the two handles do decode differently)


def test_decoder_mixed_batch_device(small):
    torch = pytest.importorskip('torch')
    with Dictionary(OTHER) as other:
        items = _mixed_sessions(small, other)
        ds = [BrotliDecoder(o) for o, _, _ in items]
        chunks = [s for _, s, _ in items]
        buf = bytearray(b'\xee' * 3 + b''.join(chunks))
        offs = [3]
        for c in chunks:
            offs.append(offs[-1] + len(c))
        room = 4096
        ooff = [5 + room * i for i in range(len(ds) + 1)]
        d_in = torch.frombuffer(buf, dtype=torch.uint8).to('cuda')
        d_out = torch.full((ooff[-1] + 5,), 0xA5, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
        sizes, st = brotli_amd.decoder_update_batch_device(ds, d_in.data_ptr(), offs, d_out.data_ptr(), ooff)
        host = d_out.cpu().numpy().tobytes()
        fsizes, fst = brotli_amd.decoder_finish_batch_device(ds, d_out.data_ptr(), ooff)
        for i, (_, _, (want, err)) in enumerate(items):
            if err is None:
                assert st[i] == 0 and fst[i] == 0 and fsizes[i] == 0, (i, st[i], fst[i])
                assert host[ooff[i]:ooff[i] + sizes[i]] == want, i
            else:
                assert st[i] in (0, err) and fst[i] == err, (i, st[i], fst[i])
        assert host[:5] == b'\xa5' * 5 and host[ooff[-1]:] == b'\xa5' * 5


def test_reference_rule_is_unchanged():
    dec = BrotliDecoder({'customDictionary': sd.DICT})
    with pytest.raises(BrotliError) as e:
        dec.update(_stream('middle')[0])
        dec.finish()
    assert e.value.code == -9


# ---------------------------------------------------------------- encoder: round trips
DOC_LEN = 600000
PIECES = (1, 70001, 300000)


def _slices_and_noise(r, n, D):
    """n bytes: slices of D (40..300 bytes, from anywhere) and noise (20..200 bytes) in turn"""
    out, size = [], 0
    while size < n:
        k = r.randrange(40, 301)
        a = r.randrange(0, len(D) - k)
        out.append(D[a:a + k])
        out.append(r.randbytes(r.randrange(20, 201)))
        size += len(out[-2]) + len(out[-1])
    return b''.join(out)[:n]


def _document():
    """600,000 bytes of slices and noise.  A session takes its input in blocks of 64 KiB (quality
    5, or lgwin 16) or 256 KiB (quality 9 and 11 at lgwin 22) and encodes the whole blocks it has
    at each update(): fed PIECES and the rest, its chunks end at 65,536 / 327,680 / 589,824 or at
    262,144 / 524,288.  Chunks start at multiples of 64 KiB, so the 64 KiB parse segments inside
    them end at multiples of 64 KiB of the stream as well.  At EVERY multiple B of 64 KiB a slice
    ends at B and another starts there -- each side of every chunk boundary and of every parse
    segment boundary, for both block lengths.  A slice lies in the first chunk (at 100), every
    slice behind 65,520 lies where the lgwin-16 window is capped, and the last bytes are a slice."""
    if 'doc' not in _built:
        r = random.Random(2024)
        D = DICT64K
        doc = bytearray(_slices_and_noise(r, DOC_LEN, D))

        def put(at, a, k):
            doc[at:at + k] = D[a:a + k]
        put(100, 30000, 180)
        for B in range(65536, DOC_LEN, 65536):
            put(B - 120, 1000 + B // 64, 120)      # ends at B
            put(B, 40000 - B // 64, 150)           # starts at B
        put(DOC_LEN - 90, 65536 - 90, 90)          # the last bytes: the dictionary's tail
        assert len(doc) == DOC_LEN
        _built['doc'] = bytes(doc)
    return _built['doc']


def _feed_encoder(enc, doc, pieces):
    out, at = [], 0
    for n in pieces:
        out.append(enc.update(doc[at:at + n]))
        at += n
    out.append(enc.update(doc[at:]))
    out.append(enc.finish())
    return b''.join(out)


def _decode_session(data, d, step=10000):
    dec = BrotliDecoder({'dictionary': d})
    out = [dec.update(data[at:at + step]) for at in range(0, len(data), step)]
    out.append(dec.finish())
    assert dec.finished
    return b''.join(out)


@pytest.mark.parametrize('mode', [EncoderMode.GENERIC, EncoderMode.FONT])
@pytest.mark.parametrize('lgwin', [16, 22])
@pytest.mark.parametrize('q', [5, 9, 11])
def test_encoder_round_trip_grid(big, q, lgwin, mode):
    doc = _document()
    enc = _feed_encoder(BrotliEncoder({'dictionary': big, 'quality': q, 'lgwin': lgwin, 'mode': mode}), doc, PIECES)
    one = brotli_amd.decode_batch([enc], dictionary=big)[0]
    assert one == doc, (q, lgwin, mode, one if isinstance(one, BrotliError) else 'bytes differ')
    assert _decode_session(enc, big) == doc, (q, lgwin, mode)


def test_encoder_throughput_mode_round_trip(big):
    """streamChunk 1 MiB: chunks of many parse segments, each with a part index, whose entries
    carry the ring that the dictionary copies before each part boundary pushed"""
    doc = _slices_and_noise(random.Random(7), 3 << 20, DICT64K)
    enc = BrotliEncoder({'dictionary': big, 'quality': 5, 'lgwin': 22, 'streamChunk': 1 << 20})
    out = [enc.update(doc[at:at + (768 << 10)]) for at in range(0, len(doc), 768 << 10)]
    out.append(enc.finish())
    data = b''.join(out)
    assert brotli_amd.decode_batch([data], dictionary=big)[0] == doc
    assert _decode_session(data, big, 100000) == doc


@pytest.mark.parametrize('mode', [EncoderMode.GENERIC, EncoderMode.FONT])
def test_ring_a_chunk_hands_on_after_a_run_of_dictionary_copies(big, mode):
    """Below max backward a run of the dictionary cut into several copies repeats ONE distance (the
    window grows as the address does), each copy coded with distance code 0 and each pushed on the
    decoder's ring.  Here a run of 900 bytes ends exactly where the first chunk ends (quality 5:
    blocks of 64 KiB; update() is given 70,000 bytes), so the ring the chunk hands to the next
    holds that distance four times over.  Before the run lies a window copy at distance 3,000, and
    the next chunk opens with another at that distance: an encoder whose carried ring still held
    3,000 in its second place would write a short code that the decoder reads as the run's
    distance."""
    r = random.Random(17)
    B = 65536
    doc = bytearray(r.randbytes(2 * B + 5000))
    doc[60000:60100] = doc[57000:57100]              # a window copy, distance 3,000
    doc[B - 900:B] = DICT64K[20000:20900]            # the run, up to the chunk's last byte
    doc[B + 20:B + 120] = doc[B + 20 - 3000:B + 120 - 3000]   # distance 3,000 again, in the next chunk
    doc[B + 300:B + 700] = DICT64K[5000:5400]        # and the dictionary again behind it
    doc = bytes(doc)
    enc = BrotliEncoder({'dictionary': big, 'quality': 5, 'lgwin': 22, 'mode': mode})
    data = enc.update(doc[:70000])
    assert len(data) > 0   # (the first chunk went out)
    data += enc.update(doc[70000:]) + enc.finish()
    one = brotli_amd.decode_batch([data], dictionary=big)[0]
    assert one == doc, one if isinstance(one, BrotliError) else 'bytes differ'
    assert _decode_session(data, big) == doc


# ---------------------------------------------------------------- the dictionary is used after the first chunk
def _late_slices_doc():
    r = random.Random(99)
    addrs = [r.randrange(0, 65536 - 200 - 150) for _ in range(200)]
    # on the CPU, before anything is concluded from sizes: no slice is a tail of the dictionary
    # (which a customDictionary session could copy too), none lies within 200 bytes of its end
    assert all(a + 150 <= 65536 - 200 for a in addrs)
    assert not any(DICT64K[a:a + 150].endswith(DICT64K[-4:]) for a in addrs)
    return r.randbytes(300000) + b''.join(DICT64K[a:a + 150] + r.randbytes(20) for a in addrs)


def test_dictionary_is_used_after_the_first_chunk(big):
    """Quality 9, lgwin 22: blocks of 256 KiB, so update() encodes the first 262,144 bytes (noise)
    and finish() the rest, which holds all 200 slices: 30,000 bytes of random data that nothing but
    the handle can shorten.  Half of that is asked for."""
    doc = _late_slices_doc()
    assert len(doc) == 334000
    opts = {'quality': 9, 'lgwin': 22}

    def run(extra):
        e = BrotliEncoder(dict(opts, **extra))
        first = e.update(doc)
        assert len(first) > 0   # (the first chunk went out: 262,144 bytes of noise)
        return first + e.finish()
    with_handle, none, custom = run({'dictionary': big}), run({}), run({'customDictionary': DICT64K})
    print('handle %d, none %d, customDictionary %d' % (len(with_handle), len(none), len(custom)))
    assert brotli_amd.decode_batch([with_handle], dictionary=big)[0] == doc
    assert _decode_session(with_handle, big) == doc
    assert len(with_handle) < len(none) - 15000
    assert not len(custom) < len(none) - 15000   # the control: a tail-only dictionary does not get there


# ---------------------------------------------------------------- encoder batch: a dictionary per job
@pytest.mark.parametrize('mode', [EncoderMode.GENERIC, EncoderMode.FONT])
def test_encoder_batch_has_a_table_per_job(big, mode):
    """five encoders with equal options in one launch sequence (quality 5: blocks of 64 KiB, so the
    200 KB fed are three blocks encoded by the batch call), a dictionary each"""
    D2 = _rand(4321, 40000)
    opts = {'quality': 5, 'lgwin': 22, 'mode': mode}
    with Dictionary(D2) as second, Dictionary(b'abc') as tiny:
        kinds = [({'dictionary': big}, DICT64K), ({'dictionary': second}, D2), ({'customDictionary': D2}, D2), ({}, None),
                 ({'dictionary': tiny}, b'abc')]
        docs = []
        for i, (_, D) in enumerate(kinds):
            r = random.Random(600 + i)
            src = D if D is not None and len(D) > 1000 else DICT64K
            body = _slices_and_noise(r, 250000, src)
            if i == 2:   # the customDictionary session: some tails of its dictionary as well
                body = body[:1000] + D2[-180:] + body[1180:100000] + D2[-60:] + body[100060:]
            docs.append(body)

        def make():
            return [BrotliEncoder(dict(opts, **extra)) for extra, _ in kinds]
        es = make()
        heads = brotli_amd.encoder_update_batch(es, [d[:200000] for d in docs])
        assert all(len(h) > 0 for h in heads)   # (the batch call did encode)
        batch = [h + e.update(d[200000:]) + e.finish() for h, e, d in zip(heads, es, docs)]
        solo = []
        for e, d in zip(make(), docs):
            solo.append(e.update(d[:200000]) + e.update(d[200000:]) + e.finish())
        assert batch == solo
        handles = [big, second, None, None, tiny]
        for i, (data, doc) in enumerate(zip(batch, docs)):
            if handles[i] is not None:
                assert brotli_amd.decode_batch([data], dictionary=handles[i])[0] == doc, i
                assert _decode_session(data, handles[i], 50000) == doc, i
            else:
                extra = {'customDictionary': D2} if i == 2 else {}
                assert brotli_amd.brotliDecode(data, extra) == doc, i


# ---------------------------------------------------------------- lifetime
def test_close_with_sessions_open():
    d = Dictionary(DICT64K)
    doc = _slices_and_noise(random.Random(31), 150000, DICT64K)
    want = _feed_encoder(BrotliEncoder({'dictionary': d, 'quality': 5}), doc, (70000,))
    enc = BrotliEncoder({'dictionary': d, 'quality': 5})
    dec = BrotliDecoder({'dictionary': d})
    head = enc.update(doc[:70000])
    out = [dec.update(head)]
    d.close()
    assert d.closed
    rest = enc.update(doc[70000:]) + enc.finish()
    assert head + rest == want
    out.append(dec.update(rest))
    out.append(dec.finish())
    assert b''.join(out) == doc and dec.finished
    with pytest.raises(ValueError):
        BrotliEncoder({'dictionary': d})
    with pytest.raises(ValueError):
        BrotliDecoder({'dictionary': d})
    del enc, dec   # (the last references: the device memory goes here)
    # the library is in order afterwards
    with Dictionary(DICT64K) as again:
        assert brotli_amd.decode_batch([want], dictionary=again)[0] == doc


# ---------------------------------------------------------------- the Node mirror
def test_node_dictionary_sessions(tmp_path, big):
    node = shutil.which('node')
    if node is None:
        pytest.skip('node is not installed')
    addon = os.path.join(ROOT, 'brotli-lib_amd', 'node', 'brotli_amd.node')
    assert os.path.exists(addon), 'run __graft_entry__.build() first'

    def b64(x):
        return base64.b64encode(x).decode()
    doc = _slices_and_noise(random.Random(55), 200000, DICT64K)
    step = 70000
    enc = BrotliEncoder({'dictionary': big, 'quality': 5, 'lgwin': 22})
    stream = b''.join([enc.update(doc[at:at + step]) for at in range(0, len(doc), step)] + [enc.finish()])
    fx = {'dictionary': b64(DICT64K), 'doc': b64(doc), 'stream': b64(stream), 'quality': 5, 'lgwin': 22, 'step': step}
    path = str(tmp_path / 'dictionary_sessions_fixture.json')
    with open(path, 'w') as f:
        json.dump(fx, f)
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'node', 'dictionary_sessions_test.js'), path], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'ALL OK' in r.stdout
