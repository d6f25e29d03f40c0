"""Batches of streaming decoder sessions (decoder_update_batch / decoder_finish_batch, DESIGN.md
§4d "Batches of sessions") against the oracle and against the same sessions driven alone.

Expected bytes and codes are the oracle's (tests/_oracle.py decode without a size, as for the
solo sessions: tests/test_gpu_stream_decode.py) and the stream model's (tests/_streams.py),
never the code under test's.  "Equals solo" compares every call's result per slot with a
BrotliDecoder fed the same chunks alone: the bytes returned, or the error's code and message.
A batch feeds its sessions in lock step; a session whose stream has run out keeps receiving b''.
"""
import base64
import hashlib
import json
import os
import random
import re

import pytest

import _inputs
import _oracle
import _streams as S
import brotli_amd

pytestmark = pytest.mark.gpu
G = _inputs.GOLDEN
WIN = 64 << 10   # the smallest outWindow

_cache = {}


def _read(*p):
    with open(os.path.join(G, *p), 'rb') as f:
        return f.read()


def _streams():
    """[(name, stream, expected)]: the solo test's corpus -- the golden vectors up to 1 MiB of
    output, the named synthetic streams, the part-indexed stream; expected is the oracle's"""
    if 'streams' not in _cache:
        out = []
        for nm in sorted(os.listdir(os.path.join(G, 'vectors'))):
            if '.compressed' in nm:
                exp = _read('vectors', nm.split('.compressed')[0])
                if len(exp) <= 1 << 20:
                    out.append((nm, _read('vectors', nm), exp))
        for st in S.named():
            out.append((st.name, S.build(st).data, S.model(st)))
        out.append(('parts_enwik300k', _read('parts', 'parts_enwik300k.br'), None))
        res = []
        for nm, data, exp in out:
            ora = _oracle.decode(data, -1)
            assert isinstance(ora, bytes), nm
            assert exp is None or exp == ora, nm
            res.append((nm, data, ora))
        _cache['streams'] = res
    return _cache['streams']


def _by_name(name):
    return next(c for c in _streams() if c[0] == name)


def _cuts_fixed(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


def _cuts_random(n, seed):
    rng = random.Random(seed)
    k = rng.randint(1, 12)
    at = sorted(rng.randrange(n + 1) for _ in range(k)) if n else []
    edges = [0] + at + [n]
    return [b - a for a, b in zip(edges, edges[1:])]   # (empty updates included)


def _chunks(data, sizes, steps):
    out, pos = [], 0
    for n in sizes:
        out.append(data[pos:pos + n])
        pos += n
    assert pos == len(data)
    return out + [b''] * (steps - len(out))


def _key(r):
    """a call's result in comparable form"""
    return ('error', r.code, str(r)) if isinstance(r, brotli_amd.BrotliError) else r


def _solo(chunks, opts):
    """(decoder, [each update's result or error], finished, finish's result or error)"""
    d = brotli_amd.BrotliDecoder(opts)
    res = []
    for c in chunks:
        try:
            res.append(d.update(c))
        except brotli_amd.BrotliError as e:
            res.append(e)
    fin = d.finished
    try:
        tail = d.finish()
    except brotli_amd.BrotliError as e:
        tail = e
    return d, res, fin, tail


def _batch(items, finish=True):
    """items: [(data, sizes, opts)].  (decoders, per session [each call's result], per session
    finished after the last update, finish_batch's results)"""
    steps = max(len(sizes) for _, sizes, _ in items)
    feeds = [_chunks(data, sizes, steps) for data, sizes, _ in items]
    ds = [brotli_amd.BrotliDecoder(opts) for _, _, opts in items]
    res = [[] for _ in items]
    for t in range(steps):
        out = brotli_amd.decoder_update_batch(ds, [f[t] for f in feeds])
        assert len(out) == len(ds)
        for i, r in enumerate(out):
            res[i].append(r)
    fin = [d.finished for d in ds]
    tails = brotli_amd.decoder_finish_batch(ds) if finish else None
    return ds, feeds, res, fin, tails


def _joined(results):
    return b''.join(r for r in results if isinstance(r, bytes))


def _assert_equals_solo(items, names, stats=False):
    ds, feeds, res, fin, tails = _batch(items)
    for i, (data, sizes, opts) in enumerate(items):
        sd, sres, sfin, stail = _solo(feeds[i], opts)
        assert [_key(r) for r in res[i]] == [_key(r) for r in sres], names[i]
        assert fin[i] == sfin and _key(tails[i]) == _key(stail), names[i]
        if stats:
            assert (ds[i].passes, ds[i].redecoded) == (sd.passes, sd.redecoded), names[i]
    return ds, res, fin, tails


def test_whole_corpus_as_one_batch():
    """every stream of the solo corpus in lock-step 4,096-byte chunks"""
    cs = _streams()
    items = [(data, _cuts_fixed(len(data), 4096), None) for _, data, _ in cs]
    ds, res, fin, tails = _assert_equals_solo(items, [c[0] for c in cs])
    for i, (nm, _, exp) in enumerate(cs):
        assert _joined(res[i]) == exp, nm
        assert fin[i] is True, nm
        assert tails[i] == b'', nm


def test_seeded_random_cuts():
    """each session its own cuts (empty updates included), outWindow 64 KiB"""
    cs = _streams()
    items = [(data, _cuts_random(len(data), 31 * i + len(nm)), {'outWindow': WIN}) for i, (nm, data, _) in enumerate(cs)]
    ds, res, fin, tails = _assert_equals_solo(items, [c[0] for c in cs], stats=True)
    for i, (nm, _, exp) in enumerate(cs):
        assert _joined(res[i]) == exp and fin[i] is True and tails[i] == b'', nm


def _batch_launches():
    import ctypes
    n = ctypes.c_uint64()
    brotli_amd._L().mib_decoder_batch_stats(ctypes.byref(n))
    return int(n.value)


def test_one_launch_per_round():
    """12 sessions of unequal need in one call: the launches are the neediest session's passes,
    not the sum"""
    _, big, big_exp = _by_name('alice29.txt.compressed')
    assert len(big_exp) > 2 * WIN
    small = [c for c in _streams() if 0 < len(c[2]) < WIN and len(c[1]) < 4096][:11]
    assert len(small) == 11
    cs = [('alice29', big, big_exp)] + small
    ds = [brotli_amd.BrotliDecoder({'outWindow': WIN}) for _ in cs]
    before = _batch_launches()
    out = brotli_amd.decoder_update_batch(ds, [c[1] for c in cs])
    made = _batch_launches() - before
    passes = [d.passes for d in ds]
    print('passes per session', passes, 'launches', made)
    assert [o for o in out] == [c[2] for c in cs]
    assert passes[0] >= 3 and all(p == 1 for p in passes[1:])   # several windows of output / one
    assert made == max(passes) and made < sum(passes)
    assert brotli_amd.decoder_finish_batch(ds) == [b''] * len(ds)


def test_solo_update_is_a_counted_launch():
    """a lone session's update() goes through the same rounds: the launch counter rises by exactly
    that session's passes (several: the stream's output is more than two windows)"""
    _, data, exp = _by_name('alice29.txt.compressed')
    d = brotli_amd.BrotliDecoder({'outWindow': WIN})
    before = _batch_launches()
    out = d.update(data)
    made = _batch_launches() - before
    assert out == exp and d.finished
    assert d.passes >= 3 and made == d.passes


def test_kernel_builds_and_grid_cap():
    """the named synthetic streams as one batch through the four-per-CU build, and with the grid
    capped at 5 blocks so that every block loops over several jobs"""
    cs = [c for c in _streams() if c[0] in {st.name for st in S.named()}]
    assert len(cs) >= 12
    lib = brotli_amd._L()
    try:
        for build, cap in ((1, 0), (0, 5), (1, 5)):
            lib.mib_force_decoder_build(build)
            lib.mib_force_decoder_grid(cap)
            items = [(data, _cuts_fixed(len(data), 4096) if cap else _cuts_random(len(data), 7 + len(nm)), None)
                     for nm, data, _ in cs]
            ds, feeds, res, fin, tails = _batch(items)
            for i, (nm, _, exp) in enumerate(cs):
                assert _joined(res[i]) == exp and fin[i] is True and tails[i] == b'', (nm, build, cap)
    finally:
        lib.mib_force_decoder_build(0)
        lib.mib_force_decoder_grid(0)


def _big(lgwin, blocks=30, size=256 << 10):
    """`blocks` uncompressed metablocks of `size` bytes and, after every fourth, a metablock of long
    copies from the far end of the window, the near end and in between (the solo test's shape)"""
    rng = random.Random(lgwin)
    s = S.State(lgwin)
    mbs = []
    for k in range(blocks):
        data = rng.randbytes(size)
        s.out += data
        mbs.append(S.MB('raw', data=data))
        if k % 4 == 3:
            cmds = []
            for _ in range(16):
                ins = rng.randbytes(3)
                s.out += ins
                spec = ('dist', rng.choice([s.maxd(), s.maxd() - 7, 1, 40000 if s.maxd() >= 40000 else 5]))
                s.copy(spec, 6000)
                cmds.append((ins, 6000, spec))
            s.out += b'.'
            cmds.append((b'.', 2, None))
            mbs.append(S.MB('cmds', cmds=cmds))
    mbs.append(S.MB('empty'))
    return S.Stream(lgwin, mbs, 'big_%d' % lgwin)


def test_history_and_input_moves_in_one_launch():
    """sessions at lgwin 10, 16, 18 and 22 with outWindow 64 KiB: their histories move in the same
    launch, overlapping (2^lgwin above what a pass adds) and not (lgwin 10: 1 KiB of history moves
    down by far more than its length), and the 8 MiB streams' pending input is compacted"""
    sts = [(S.ring_wrap(), 1000), (S.transitions(lgwin=16), 1000), (S.transitions(lgwin=18), 1000),
           (S.transitions(lgwin=22), 1000), (_big(16), 1 << 20), (_big(22), 1 << 20),
           (_big(10, blocks=12, size=60000), 100000)]
    items, exps = [], []
    for st, chunk in sts:
        data, exp = S.build(st).data, S.model(st)
        assert _oracle.decode(data, -1) == exp, st.name
        items.append((data, _cuts_fixed(len(data), chunk), {'outWindow': WIN}))
        exps.append(exp)
    assert len(exps[4]) >= 8 << 20 and len(exps[5]) >= 8 << 20 and len(exps[6]) > 10 * WIN
    ds, feeds, res, fin, tails = _batch(items)
    for i, (st, _) in enumerate(sts):
        assert _joined(res[i]) == exps[i], st.name
        assert fin[i] is True and tails[i] == b'', st.name
    print('device passes', [d.passes for d in ds])
    for i in (4, 5):   # beyond one per update: the window moved
        assert ds[i].passes >= 8 + len(items[i][1]), sts[i][0].name
    assert ds[6].passes > len(items[6][1])   # (two 60,000-byte metablocks fill a window: fewer, longer passes)


def test_dictionaries():
    """tests/golden/decode_compound.json, 64 sessions per batch in 13-byte chunks, every eighth
    slot a session without a dictionary"""
    with open(os.path.join(G, 'decode_compound.json')) as f:
        cases = json.load(f)['cases']
    _, plain, plain_exp = _by_name('10x10y.compressed')
    n = 0
    for b0 in range(0, len(cases), 56):
        group = cases[b0:b0 + 56]
        items, what = [], []
        for i, c in enumerate(group):
            if i % 7 == 0:
                items.append((plain, _cuts_fixed(len(plain), 13), None))
                what.append(None)
            data = base64.b64decode(c['in_b64'])
            items.append((data, _cuts_fixed(len(data), 13), {'customDictionary': _inputs.resolve(c['dict'])}))
            what.append(c)
        assert len(items) <= 64
        ds, feeds, res, fin, tails = _batch(items)
        for i, c in enumerate(what):
            errs = [r for r in res[i] + [tails[i]] if isinstance(r, brotli_amd.BrotliError)]
            got = errs[0].code if errs else hashlib.sha256(_joined(res[i] + [tails[i]])).hexdigest()
            if c is None:
                assert not errs and _joined(res[i]) == plain_exp and fin[i]
            elif 'error' not in c:
                assert got == c['sha256'] and fin[i], c
                n += 1
            elif c['error'].startswith('Brotli error code'):
                assert got == int(re.search(r'-\d+', c['error']).group()), (c, got)
            else:
                assert got == -106, (c, got)   # MIB_E_JS_TYPE_ERROR: the reference's TypeError
    assert n > 100


def _outcome(results, tail):
    """what a slot ends in: the first error's code, or the joined bytes; and asserts that a
    failed session reports its code again in every later call"""
    calls = results + [tail]
    for t, r in enumerate(calls):
        if isinstance(r, brotli_amd.BrotliError):
            assert all(isinstance(x, brotli_amd.BrotliError) and x.code == r.code for x in calls[t:])
            return r.code, _joined(calls[:t])
    return _joined(calls), _joined(calls)


def test_error_isolation():
    """decode_errors.json in batches of 64: each corruption between two valid sessions"""
    with open(os.path.join(G, 'decode_errors.json')) as f:
        cases = json.load(f)['cases']
    _, valid, valid_exp = _by_name('alice29.txt.compressed')
    two = lambda data: [len(data) // 2, len(data) - len(data) // 2]
    n = failed = failed_early = 0
    for b0 in range(0, len(cases), 31):
        group = [base64.b64decode(c['in_b64']) for c in cases[b0:b0 + 31]]
        items = [(valid, two(valid), None)]
        for data in group:
            items += [(data, two(data), None), (valid, two(valid), None)]
        assert len(items) <= 64
        ds, feeds, res, fin, tails = _batch(items)
        for i, (data, _, _) in enumerate(items):
            got, _ = _outcome(res[i], tails[i])
            if i % 2 == 0:   # the neighbours: complete, whatever happened beside them
                assert got == valid_exp and fin[i] is True and tails[i] == b''
                continue
            exp = _oracle.decode(data, -1)
            assert got == exp, (b0, i, got if isinstance(got, int) else len(got))
            n += 1
            if isinstance(got, int):
                failed += 1
                failed_early += isinstance(res[i][0], brotli_amd.BrotliError)
    print('corruptions', n, 'failed', failed, 'of which in the first of the two updates', failed_early)
    assert n > 700 and failed > 500 and failed_early >= 1


TRUNCATED = ('alice29.txt.compressed', 'mapsdatazrh.compressed', 'monkey.compressed', 'transitions', 'placed_words_40000')


def test_truncations_and_trailing_bytes():
    """the five streams cut at eight seeded offsets each, all 40 in one batch, then
    decoder_finish_batch; and trailing bytes, which fail their own slot only"""
    rng = random.Random(17)
    items, full = [], []
    for name in TRUNCATED:
        _, data, exp = _by_name(name)
        for _ in range(8):
            cut = rng.randrange(len(data))
            split = rng.randrange(cut + 1)
            items.append((data[:cut], [split, cut - split], None))
            full.append(exp)
    ds, feeds, res, fin, tails = _batch(items)
    for i, (data, _, _) in enumerate(items):
        got, before = _outcome(res[i], tails[i])
        assert got == _oracle.decode(data, -1), i
        assert full[i].startswith(before), i
    items, full = [], []
    for name in TRUNCATED:
        _, data, exp = _by_name(name)
        for extra, sizes in ((1, [len(data), 1]), (100, [len(data) - 1, 101]), (100, [len(data) + 100, 0])):
            items.append((data, [len(data), 0], None))
            full.append(exp)
            more = data + bytes(range(1, extra + 1))
            assert _oracle.decode(more, -1) == -17, name
            items.append((more, sizes, None))
            full.append(-17)
    ds, feeds, res, fin, tails = _batch(items)
    for i in range(len(items)):
        got, before = _outcome(res[i], tails[i])
        assert got == full[i], i
        if full[i] == -17:
            assert full[i - 1].startswith(before)


def test_max_output_size():
    _, data, full = _by_name('alice29.txt.compressed')
    sizes = _cuts_fixed(len(data), 4096)
    limits = [len(full) - 1, len(full), None]
    items = [(data, sizes, {'maxOutputSize': m} if m is not None else None) for m in limits]
    ds, feeds, res, fin, tails = _batch(items)
    got, _ = _outcome(res[0], tails[0])
    assert got == -103   # MIB_E_OUTPUT_LIMIT
    err = next(r for r in res[0] if isinstance(r, brotli_amd.BrotliError))
    assert str(err) == 'Decompressed size %d exceeds limit %d' % (len(full), len(full) - 1)   # the reference's message
    for i in (1, 2):
        assert _outcome(res[i], tails[i])[0] == full and fin[i]
    # ... as the solo session words it
    _, sres, _, _ = _solo(feeds[0], items[0][2])
    assert [_key(r) for r in res[0]] == [_key(r) for r in sres]


def test_interleaving_and_other_entry_points():
    """a session alternates solo update() and batch calls; one-shot and batch decoding work
    between batch calls with sessions open"""
    _, data, full = _by_name('alice29.txt.compressed')
    _, other, other_full = _by_name('mapsdatazrh.compressed')
    plain = b'The quick brown fox jumps over the lazy dog. ' * 300
    enc = brotli_amd.brotliEncode(plain, {'quality': 5})
    a = brotli_amd.BrotliDecoder({'outWindow': WIN})
    b = brotli_amd.BrotliDecoder()
    got_a, got_b = [], []
    pieces = _chunks(data, _cuts_fixed(len(data), 3000), 0)
    others = _chunks(other, _cuts_fixed(len(other), 3000), len(pieces))
    for t, piece in enumerate(pieces):
        if t % 2:
            got_a.append(a.update(piece))
            got_b.append(b.update(others[t]))
        else:
            ra, rb = brotli_amd.decoder_update_batch([a, b], [piece, others[t]])
            got_a.append(ra)
            got_b.append(rb)
        if t == 3:
            assert brotli_amd.brotliDecode(data) == full
            assert brotli_amd.decode_batch([data, enc, data]) == [full, plain, full]
    assert b''.join(got_a) == full and a.finished
    got_b.append(b.update(b''.join(others[len(pieces):])))
    assert b''.join(got_b) == other_full and b.finished
    assert brotli_amd.decoder_finish_batch([a, b]) == [b'', b'']
    assert brotli_amd.brotliDecode(enc) == plain


# kGatherTile = 4096 bytes; 1 MiB + 1 is the first length whose tiles exceed kGatherSpread = 256
# blocks, so a block of the copy launch walks more than one tile
DELIVERY_SIZES = (1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 1)
DELIVERY_HEAD = 5   # the first metablock's bytes: odd, so what follows starts off a 16-byte granule


def test_host_delivery_through_the_copy_kernel():
    """host delivery at the sizes where the copy launch can go wrong: one call whose sessions'
    single launch decodes 1 ... 1 MiB + 1 bytes (under, at and over a 16-byte granule and a tile;
    more tiles than blocks), then the same streams in two chunks each, cut inside their second
    uncompressed metablock, so that the second call's bytes start at `deliv` = 5 in the session
    buffer.  Every byte against the plaintext."""
    assert ((1 << 20) + 4095) // 4096 == 256 and ((1 << 20) + 1 + 4095) // 4096 > 256
    rng = random.Random(12)
    plains, datas = [], []
    for n in DELIVERY_SIZES:
        plain = rng.randbytes(n)
        parts = [plain[:DELIVERY_HEAD], plain[DELIVERY_HEAD:]]
        st = S.Stream(22, [S.MB('raw', data=p) for p in parts if p] + [S.MB('empty')])
        assert S.model(st) == plain
        plains.append(plain)
        datas.append(S.build(st).data)
    ds = [brotli_amd.BrotliDecoder() for _ in datas]
    before = _batch_launches()
    out = brotli_amd.decoder_update_batch(ds, datas)
    assert _batch_launches() - before == 1 and all(d.passes == 1 for d in ds)
    assert [len(o) for o in out] == list(DELIVERY_SIZES)
    assert out == plains
    assert all(d.finished for d in ds) and brotli_amd.decoder_finish_batch(ds) == [b''] * len(ds)
    # two chunks: the cut leaves the last byte of the second metablock (and the stream's end) out
    cuts = [len(data) - 1 - (max(len(plain) - DELIVERY_HEAD, 0) + 1) // 2 for data, plain in zip(datas, plains)]
    ds = [brotli_amd.BrotliDecoder() for _ in datas]
    first = brotli_amd.decoder_update_batch(ds, [data[:c] for data, c in zip(datas, cuts)])
    second = brotli_amd.decoder_update_batch(ds, [data[c:] for data, c in zip(datas, cuts)])
    for n, plain, a, b in zip(DELIVERY_SIZES, plains, first, second):
        if n > DELIVERY_HEAD:   # an uncompressed metablock comes whole or not at all
            assert a == plain[:DELIVERY_HEAD], n
        assert a + b == plain, n
    assert all(d.finished for d in ds) and brotli_amd.decoder_finish_batch(ds) == [b''] * len(ds)
