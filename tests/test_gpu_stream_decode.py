"""The streaming decoder (BrotliDecoder.update / finish / finished) against the
oracle: every way of cutting a stream into updates gives the bytes one-shot decoding gives,
suspending inside commands and headers, moving its output window, with a dictionary, and
failing with the reference decoder's codes.

Expected bytes and codes are the oracle's (tests/_oracle.py decode), the synthetic streams'
also the model's (tests/_streams.py model), never the code under test's.  A streaming decoder
cannot know a stream's size, so the oracle is asked without one (out_size = -1): with a size
from the header the reference stops when the buffer is full and skips its checks behind the
last byte.  Where tests/golden/decode_errors.json records an error the two agree (asserted
below); 92 of its corruptions "decode" only because of that skipped check, and there the
expected code is the oracle's without a size (-13, -17, -5).

Launch counts.  Every update() is at least one launch, and a resumed launch re-reads its
metablock's header (1-9 ms for the largest: many_types has 768 block types), so the 7-byte
chunking is 400 updates of 7 bytes per stream: the first 200 from the stream's start and 200
more from a seeded offset deep in it, the bytes between and after in 4,096-byte updates (a
stream of up to 2,800 bytes is in 7-byte updates throughout).  1-byte updates run for the
streams of at most 512 bytes only.  Every other chunking is as listed.

Bytes before an error.  What update() returned before a session failed must be what the
reference had decoded at that point.  For a cut-off valid stream that is a prefix of the whole
stream's output.  For a corruption the oracle is asked with that many bytes as the size: with a
size it stops at the full buffer, so it returns exactly its first len(before) bytes -- where
it has flushed them.  The reference flushes its ring at the fence and at the stream's end only,
so where it fails before its first flush it returns no bytes for any size and the oracle
cannot confirm them; the test counts both kinds and requires the confirmed kind to occur.
(On an MI355X: 706 corruptions, 106 with bytes returned before the error, 42 of those
confirmed byte for byte, 64 where the oracle has nothing to show; 9 of the truncations.)
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
    """[(name, stream, expected)]: the golden vectors up to 1 MiB of output, the named synthetic
    streams, and the part-indexed stream (it opens with a metadata block)"""
    if 'streams' not in _cache:
        out = []
        for nm in sorted(os.listdir(os.path.join(G, 'vectors'))):
            if '.compressed' in nm:
                exp = _read('vectors', nm.split('.compressed')[0])
                if len(exp) <= 1 << 20:
                    out.append((nm, _read('vectors', nm), exp))
        for st in S.named():
            data = S.build(st).data
            exp = S.model(st)
            if exp is None:
                exp = _oracle.decode(data, -1)
            out.append((st.name, data, exp))
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


def _cuts_seven(n, seed=0):
    if n <= 7 * 400:
        return _cuts_fixed(n, 7)
    run = 7 * 200
    deep = random.Random(seed).randrange(run + (n - 2 * run) // 2, n - run + 1)   # in the stream's second half
    return _cuts_fixed(run, 7) + _cuts_fixed(deep - run, 4096) + _cuts_fixed(run, 7) + _cuts_fixed(n - deep - run, 4096)


def _cuts_random(n, seed):
    rng = random.Random(seed)
    k = rng.randint(1, 12)
    at = sorted(rng.randrange(n + 1) for _ in range(k)) if n else []
    edges = [0] + at + [n]
    return [b - a for a, b in zip(edges, edges[1:])]   # (empty updates included)


def _feed(data, sizes, opts=None):
    """(decoder, [update results])"""
    d = brotli_amd.BrotliDecoder(opts)
    outs, pos = [], 0
    for n in sizes:
        outs.append(d.update(data[pos:pos + n]))
        pos += n
    assert pos == len(data)
    return d, outs


def _decode(data, sizes, opts=None):
    d, outs = _feed(data, sizes, opts)
    fin = d.finished
    tail = d.finish()
    return b''.join(outs), fin, tail, d


CHUNKINGS = ['one', 'b7x400', 'b4096', 'b65536', 'rand1', 'rand2', 'rand3']


def _names():
    """the ids of _streams(), without decoding anything (collection runs everywhere)"""
    out = [nm for nm in sorted(os.listdir(os.path.join(G, 'vectors')))
           if '.compressed' in nm and os.path.getsize(os.path.join(G, 'vectors', nm.split('.compressed')[0])) <= 1 << 20]
    return out + [st.name for st in S.named()] + ['parts_enwik300k']


def _names_small():
    """the streams of at most 512 bytes (the named ones are built for their size: 0.6 s)"""
    out = [nm for nm in _names() if '.compressed' in nm and os.path.getsize(os.path.join(G, 'vectors', nm)) <= 512]
    return out + [st.name for st in S.named() if len(S.build(st).data) <= 512]


def _check(data, sizes, exp):
    assert sum(sizes) == len(data)
    got, fin, tail, _ = _decode(data, sizes)
    assert got == exp
    assert fin is True   # after the last byte, before finish()
    assert tail == b''


@pytest.mark.parametrize('chunking', CHUNKINGS)
@pytest.mark.parametrize('name', _names())
def test_chunkings(name, chunking):
    _, data, exp = _by_name(name)
    n = len(data)
    if chunking == 'one':
        sizes = [n]
    elif chunking == 'b7x400':
        sizes = _cuts_seven(n, len(name))
    elif chunking.startswith('b'):
        sizes = _cuts_fixed(n, int(chunking[1:]))
    else:
        sizes = _cuts_random(n, 100 * int(chunking[4:]) + len(name))
    _check(data, sizes, exp)


@pytest.mark.parametrize('name', _names_small())
def test_one_byte_updates(name):
    _, data, exp = _by_name(name)
    assert len(data) <= 512
    _check(data, [1] * len(data), exp)


def test_one_byte_updates_cover_every_small_stream():
    assert sorted(_names_small()) == sorted(nm for nm, data, _ in _streams() if len(data) <= 512)


@pytest.mark.parametrize('name', [st.name for st in S.named()])
def test_four_per_cu_build(name):
    """The named streams through the decode kernel's four-per-CU build (12,224 LDS table entries,
    block-type trees in scratch), which a lone session does not get by itself: the table-size
    boundaries 12,224 / 12,225 are this build's, and past them it decodes from the HBM tables."""
    _, data, exp = _by_name(name)
    lib = brotli_amd._L()
    lib.mib_force_decoder_build(1)
    try:
        _check(data, _cuts_fixed(len(data), 4096), exp)
        _check(data, _cuts_random(len(data), 7 + len(name)), exp)
    finally:
        lib.mib_force_decoder_build(0)


def test_every_cut():
    """two updates, cut at every byte offset"""
    for name in ('10x10y.compressed', '64x.compressed', 'simple_codes'):
        _, data, exp = _by_name(name)
        for cut in range(len(data) + 1):
            got, fin, tail, _ = _decode(data, [cut, len(data) - cut])
            assert (got, fin, tail) == (exp, True, b''), (name, cut)


def _lit_run():
    rng = random.Random(1)
    lits = bytes(rng.choice(b'abcdefghijklmnop') for _ in range(20000))
    return S.Stream(18, [S.MB('cmds', cmds=[(lits[:9000], 5, ('dist', 3)), (lits[9000:], 2, None)])], 'lit_run')


def _raw_mid():
    rng = random.Random(2)
    raw = bytes(rng.randrange(256) for _ in range(3000))
    return S.Stream(16, [S.MB('cmds', cmds=[(b'ab', 3, ('dist', 1)), (b'c', 2, None)]), S.MB('raw', data=raw),
                         S.MB('cmds', cmds=[(b'xy', 4, ('dist', 2000)), (b'z', 2, None)]), S.MB('empty')], 'raw_mid')


@pytest.mark.parametrize('which', ['long_run', 'lit_run', 'raw_mid'])
def test_suspend_inside_commands_and_headers(which):
    """64-byte updates: a command of thousands of literals, an uncompressed metablock.  While
    one is incomplete the decoder has input it cannot act on: update() returns nothing and keeps
    its last checkpoint (rule 1).  (_streams.long_run's commands are long copies, and the whole
    stream is 14 bytes: it is decoded here too, but only lit_run and raw_mid can starve.)"""
    st = {'long_run': S.long_run((1 << 20) + 5), 'lit_run': _lit_run(), 'raw_mid': _raw_mid()}[which]
    data = S.build(st).data
    exp = S.model(st)
    assert _oracle.decode(data, -1) == exp
    d, outs = _feed(data, _cuts_fixed(len(data), 64))
    assert b''.join(outs) == exp and d.finished and d.finish() == b''
    starved = sum(1 for o in outs[:-1] if not o)
    print(which, 'updates', len(outs), 'with no output', starved)
    if which != 'long_run':
        assert len(data) > 640 and starved >= 1


def _big(lgwin):
    """30 uncompressed metablocks of 256 KiB and, after every fourth, a metablock of long copies
    from the far end of the window, the near end and in between: 8.1 MiB"""
    rng = random.Random(lgwin)
    s = S.State(lgwin)
    mbs = []
    for k in range(30):
        data = rng.randbytes(256 << 10)
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


@pytest.mark.parametrize('lgwin', [16, 18, 22])
def test_rebasing_and_compaction(lgwin):
    """outWindow 64 KiB: the history moves to the front of the session buffer again and again,
    copies reach the far end of the window across the moves"""
    small = [S.ring_wrap(), S.transitions(lgwin=lgwin), S.many_types(lgwin=lgwin)]
    for st in small:
        data, exp = S.build(st).data, S.model(st)
        got, fin, tail, _ = _decode(data, _cuts_fixed(len(data), 1000), {'outWindow': WIN})
        assert (got, fin, tail) == (exp, True, b''), st.name
    st = _big(lgwin)
    data, exp = S.build(st).data, S.model(st)
    assert len(exp) >= 8 << 20 and _oracle.decode(data, -1) == exp
    got, fin, tail, d = _decode(data, _cuts_fixed(len(data), 1 << 20), {'outWindow': WIN})
    assert got == exp and fin and tail == b''
    print('lgwin', lgwin, 'device passes', d.passes)
    assert d.passes >= 8 + len(data) // (1 << 20)   # beyond one per update: the window moved


def test_dictionary():
    """tests/golden/decode_compound.json in 13-byte updates with its dictionary"""
    with open(os.path.join(G, 'decode_compound.json')) as f:
        cases = json.load(f)['cases']
    n = 0
    for c in cases:
        data = base64.b64decode(c['in_b64'])
        dic = _inputs.resolve(c['dict'])
        try:
            got, fin, tail, _ = _decode(data, _cuts_fixed(len(data), 13), {'customDictionary': dic})
            got = hashlib.sha256(got + tail).hexdigest()
        except brotli_amd.BrotliError as e:
            got = e.code
        if 'error' not in c:
            assert got == c['sha256'] and fin, c
            n += 1
        elif c['error'].startswith('Brotli error code'):
            assert got == int(re.search(r'-\d+', c['error']).group()), (c, got)
        else:
            assert got == -106, (c, got)   # MIB_E_JS_TYPE_ERROR: the reference's TypeError
    assert n > 100


def _code(data, sizes, opts=None):
    """(what the session ends in: the error code or the bytes, the bytes returned before)"""
    d = brotli_amd.BrotliDecoder(opts)
    outs, pos = [], 0
    try:
        for k in sizes:
            outs.append(d.update(data[pos:pos + k]))
            pos += k
        outs.append(d.finish())
    except brotli_amd.BrotliError as e:
        # every later call reports the same code
        for call in (lambda: d.update(b'x'), d.finish):
            with pytest.raises(brotli_amd.BrotliError) as again:
                call()
            assert again.value.code == e.code
        return e.code, b''.join(outs)
    return b''.join(outs), b''.join(outs)


def _confirm_prefix(data, before, what):
    """1 when the oracle, asked for len(before) bytes of `data`, returns them (they must be
    `before`); 0 when it fails before its first flush and has no bytes to show (module docstring)"""
    ref = _oracle.decode(data, len(before))
    if isinstance(ref, int):
        return 0
    assert ref == before, what
    return 1


def test_error_corpus():
    """the corruptions of decode_errors.json (all are under 64 KiB), in two updates"""
    with open(os.path.join(G, 'decode_errors.json')) as f:
        cases = json.load(f)['cases']
    n = early = confirmed = 0
    for c in cases:
        data = base64.b64decode(c['in_b64'])
        assert len(data) <= 64 << 10
        exp = _oracle.decode(data, -1)
        if 'error' in c and not c.get('hang'):
            assert exp == int(re.search(r'-\d+', c['error']).group()), c['in_b64'][:60]
        got, before = _code(data, [len(data) // 2, len(data) - len(data) // 2])
        assert got == exp, (c['in_b64'][:60], got if isinstance(got, int) else len(got), exp if isinstance(exp, int) else len(exp))
        n += 1
        if isinstance(got, int) and before:
            early += 1
            confirmed += _confirm_prefix(data, before, c['in_b64'][:60])
    print('corruptions', n, 'with bytes before the error', early, 'of which the oracle confirms', confirmed)
    assert n > 700 and confirmed >= 1


TRUNCATED = ('alice29.txt.compressed', 'mapsdatazrh.compressed', 'monkey.compressed', 'transitions', 'placed_words_40000')


def test_truncations():
    """five streams cut at 40 seeded offsets, then finish(): the oracle's code for those bytes,
    and whatever was returned before it is a prefix of the whole stream's output"""
    rng = random.Random(17)
    confirmed = 0
    for name in TRUNCATED:
        _, data, full = _by_name(name)
        for _ in range(40):
            cut = rng.randrange(len(data))
            exp = _oracle.decode(data[:cut], -1)
            split = rng.randrange(cut + 1)
            got, before = _code(data[:cut], [split, cut - split])
            assert got == exp, (name, cut)
            assert full.startswith(before), (name, cut)
            if before:
                confirmed += _confirm_prefix(data[:cut], before, (name, cut))
    print('truncations whose returned bytes the oracle confirms too', confirmed)


def test_trailing_bytes():
    for name in TRUNCATED:
        _, data, full = _by_name(name)
        for extra in (1, 100):
            more = data + bytes(range(1, extra + 1))
            exp = _oracle.decode(more, -1)
            assert isinstance(exp, int), name
            for sizes in ([len(more)], [len(data), extra], [len(data) - 1, 1 + extra]):
                got, before = _code(more, sizes)
                assert got == exp, (name, extra, sizes)
                assert full.startswith(before)


def test_output_limit():
    _, data, full = _by_name('alice29.txt.compressed')
    got, _ = _code(data, _cuts_fixed(len(data), 4096), {'maxOutputSize': len(full) - 1})
    assert got == -103   # MIB_E_OUTPUT_LIMIT
    got, _ = _code(data, _cuts_fixed(len(data), 4096), {'maxOutputSize': len(full)})
    assert got == full


def test_solo_trace_is_the_parents():
    """tests/golden/stream_solo_trace.json (scripts/record_stream_trace.py, recorded from the
    library of the commit it names, the last with a loop of its own for a lone session): every
    stream of at most 256 KiB compressed, alone through update() / finish() in 4,096-byte chunks
    and with seeded cuts at outWindow 64 KiB.  What only the host loop determines is the
    recording's -- the length of every call's return (so, the bytes held back until the next
    call), passes and redecoded -- and the joined bytes are the oracle's."""
    with open(os.path.join(G, 'stream_solo_trace.json')) as f:
        rec = {(c['name'], c['schedule']): c for c in json.load(f)['cases']}
    n = 0
    for i, (name, data, exp) in enumerate(_streams()):
        if len(data) > 256 << 10:
            continue
        for schedule, sizes, opts in (('b4096', _cuts_fixed(len(data), 4096), None),
                                      ('rand', _cuts_random(len(data), 31 * i + len(name)), {'outWindow': WIN})):
            c = rec.pop((name, schedule))
            d, outs = _feed(data, sizes, opts)
            outs.append(d.finish())
            assert [len(o) for o in outs] == c['lens'], (name, schedule)
            assert (d.passes, d.redecoded) == (c['passes'], c['redecoded']), (name, schedule)
            assert b''.join(outs) == exp, (name, schedule)
            n += 1
    assert not rec and n == 164   # every recorded case, and the corpus has no stream the recording lacks


def test_existing_paths_after_a_session():
    """the default context's state: one-shot and batch decoding after sessions have run, and
    with one still open"""
    _, data, full = _by_name('alice29.txt.compressed')
    d = brotli_amd.BrotliDecoder()
    first = d.update(data[:20000])
    assert brotli_amd.brotliDecode(data) == full
    plain = b'The quick brown fox jumps over the lazy dog. ' * 300
    enc = brotli_amd.brotliEncode(plain, {'quality': 5})
    assert brotli_amd.decode_batch([data, enc, data]) == [full, plain, full]
    assert first + d.update(data[20000:]) + d.finish() == full
    assert brotli_amd.brotliDecode(enc) == plain
