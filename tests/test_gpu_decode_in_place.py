"""Decoding in the output slot (decode_core.inc maybe_realloc_ring, kDirectRing / kDirectSlot).

A stream that is one final compressed metablock decodes straight into its slot when the slot
holds what the stream announces plus MIB_IN_PLACE_SLACK bytes (or the reference's whole ring);
every other stream, and every smaller slot, goes through the scratch ring.  The bytes, sizes and
error codes are the oracle's either way; which way a stream went is read back from the debug
counter (brotli_amd.in_place_stats).

Which streams are eligible is restated here from the stream alone (_in_place below): the
metablock list is the oracle's trace, the ring size the reference's arithmetic.

Every output tensor is filled with a sentinel and ends in 4 MiB of it, so a store outside a slot
lands in memory the test owns and shows up in a comparison.
"""
import random

import pytest

import _oracle
import _streams as S
import brotli_amd
from test_gpu_decode_synthetic import _cases, _corrupted, _cus

pytestmark = pytest.mark.gpu

SLACK = brotli_amd.IN_PLACE_SLACK
SENT = 0xA5
TAIL = 4 << 20
LEAD = 4096
# a dictionary word may end this far past the announced total (inside the slot's slack)
WORD_OVERSHOOT = 36

_cache = {}


def _text(n, seed):
    rng = random.Random(seed)
    words = [b'the', b'quick', b'brown', b'fox', b'jumps', b'over', b'lazy', b'dog', b'decoder', b'window',
             b'metablock', b'literal', b'distance', b'\xc3\xa9t\xc3\xa9', b'na\xc3\xafve', b'2024', b'ring,', b'slot.']
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b' ' if rng.random() < 0.9 else b'\n')
    return bytes(out[:n])


def _ring(lgwin, total):
    """the reference's ring size for a stream whose first metablock is final (engine.ts:608-630)"""
    ns = 1 << lgwin
    if ns > total:
        while (ns >> 1) > total:
            ns >>= 1
    return ns


def _in_place(lgwin, total, slot, single):
    """the rule: one final compressed metablock, and the whole ring or the announced total fits
    the slot: 'done', or 'left' where the whole ring fits but the stream outgrows it (it begins
    in place and goes back to the scratch ring when the ring wraps), or None"""
    if not single or total == 0:
        return None
    ns = _ring(lgwin, total)
    if total <= ns:
        return 'done' if ns + 37 + 64 <= slot or total + SLACK <= slot else None
    return 'left' if ns + 37 + 64 <= slot else None


def _lgwin(data):
    """window bits of a stream header (RFC 7932 section 9.1)"""
    b = data[0] | (data[1] << 8 if len(data) > 1 else 0)
    if b & 1 == 0:
        return 16
    n = (b >> 1) & 7
    if n:
        return 17 + n
    n = (b >> 4) & 7
    return 17 if n == 0 else 8 + n


def _single(data):
    return tuple(_oracle.trace(data)['metablocks']) == (1, 0, 0, 0)


def _tiny(n):
    """n bytes in one final compressed metablock (the encoder stores inputs this small)"""
    st = S.Stream(22, [S.MB('cmds', cmds=[(b'xyz'[:n], 2, None)])], 'tiny_%d' % n)
    b = S.build(st)
    assert S.model(st) == b'xyz'[:n]
    return b.data, b'xyz'[:n]


def _valid():
    """[(name, stream, expected, lgwin, single metablock)]: the issue's sizes at q11 and q5,
    and 1..3 bytes as written compressed metablocks"""
    if 'valid' not in _cache:
        out = []
        for q in (11, 5):
            for n in (1, 2, 3, 65535, 65536, 65537, 100000):
                data = _text(n, 100 * q + n % 97)
                enc = brotli_amd.brotliEncode(data, {'quality': q, 'lgwin': 22})
                assert _oracle.decode(enc) == data
                out.append(('q%d_%d' % (q, n), enc, data, _lgwin(enc), _single(enc)))
        for n in (1, 2, 3):
            enc, data = _tiny(n)
            assert _oracle.decode(enc) == data
            out.append(('tiny_%d' % n, enc, data, 22, _single(enc)))
        assert sum(1 for c in out if c[4]) >= 11
        _cache['valid'] = out
    return _cache['valid']


def _decode(cases, slots, ctx=None):
    """cases through DeviceContext.decode, stream k in a slot of slots[k] bytes, the slots packed
    behind LEAD sentinel bytes: (sizes, statuses, the slots' bytes, (finished, left) in place).
    Asserts the sentinel before the first and behind the last slot."""
    import torch
    dev = torch.device('cuda', 0)
    ioff, ooff = [0], [LEAD]
    for c, slot in zip(cases, slots):
        ioff.append(ioff[-1] + len(c[1]))
        ooff.append(ooff[-1] + slot)
    src = torch.frombuffer(bytearray(b''.join(c[1] for c in cases) + bytes(16)), dtype=torch.uint8).to(dev)
    out = torch.full((ooff[-1] + TAIL,), SENT, dtype=torch.uint8, device=dev)
    ctx = ctx or brotli_amd.DeviceContext(0)
    sizes, status = ctx.decode(src.data_ptr(), ioff, out.data_ptr() + LEAD, [o - LEAD for o in ooff])
    torch.cuda.synchronize()
    stats = brotli_amd.in_place_stats(ctx)
    host = out.cpu().numpy().tobytes()
    assert host[:LEAD] == bytes([SENT]) * LEAD, 'a store before the first slot'
    assert host[ooff[-1]:] == bytes([SENT]) * TAIL, 'a store behind the last slot'
    return sizes, status, [host[ooff[k]:ooff[k + 1]] for k in range(len(cases))], stats


def _check_valid(cases, slots, got):
    sizes, status, bufs, stats = got
    want = left = 0
    for k, (c, slot) in enumerate(zip(cases, slots)):
        name, _, exp, lgwin, single = c[:5]
        assert status[k] == 0 and sizes[k] == len(exp), (name, slot, status[k], sizes[k])
        assert bufs[k][:len(exp)] == exp, (name, slot)
        # nothing but a dictionary word's end lies behind the result
        assert bufs[k][len(exp) + WORD_OVERSHOOT:] == bytes([SENT]) * (slot - len(exp) - WORD_OVERSHOOT), (name, slot)
        how = _in_place(lgwin, len(exp), slot, single)
        want += how == 'done'
        left += how == 'left'
    assert stats == (want, left), (stats, want, left)
    return want


def _batch_of(cases):
    """more streams than CUs (the batch build): the cases repeated and shuffled"""
    n = 2 * _cus() + 3
    assert n <= 2048
    picked = [cases[i % len(cases)] for i in range(n)]
    random.Random(5).shuffle(picked)
    return picked


SLOT_RULES = {'bench': lambda n: n + 4096, 'slack': lambda n: n + SLACK, 'short': lambda n: n + SLACK - 1}


@pytest.mark.parametrize('rule', sorted(SLOT_RULES))
@pytest.mark.parametrize('build', ['big', 'batch'])
def test_sizes_and_slots(build, rule):
    """bytes, sizes, statuses, sentinels and the in-place count: every eligible stream in place
    with the bench's slots and with size + slack, none with one byte less"""
    cases = _valid() if build == 'big' else _batch_of(_valid())
    assert (len(cases) <= _cus()) == (build == 'big')
    slots = [SLOT_RULES[rule](len(c[2])) for c in cases]
    want = _check_valid(cases, slots, _decode(cases, slots))
    eligible = sum(1 for c in cases if c[4])
    assert want == (0 if rule == 'short' else eligible)


def _ctx_stream(mode, seed):
    """the first two literals are modelled on the zero bytes at positions -1 and -2: 64 literal
    trees, one per context, each with the symbols of its own context only"""
    rng = random.Random(seed)
    s = S.State(22)
    alphabet = b'Aa \xc3\xa9\x80\xff\x00z.9' if mode == S.UTF8 else bytes([0, 1, 15, 16, 63, 64, 127, 128, 191, 192, 240, 255])
    mb = S.MB('cmds')
    first = bytes(rng.choice(alphabet) for _ in range(5))
    s.out += first
    s.copy(('dist', 2), 3)
    mb.cmds = [(first, 3, ('dist', 2))] + S.gen_cmds(rng, s, 40, alphabet)
    mb.modes = [mode]
    mb.ntrees_l, mb.lmap = 64, list(range(64))
    st = S.Stream(22, [mb], 'ctx_%d_%d' % (mode, seed), seed)
    b = S.build(st)
    exp = S.model(st)
    assert exp is not None and _oracle.decode(b.data) == exp
    # the trees in use differ: the context of a literal decides which code reads it
    assert len({k for k in b.stats['trees_used'] if k[0] == 'L'}) > 4
    return (st.name, b.data, exp, 22, True)


@pytest.mark.parametrize('build', ['big', 'batch'])
def test_zero_context_at_the_start(build):
    cases = [_ctx_stream(mode, seed) for mode in (S.UTF8, S.SIGNED) for seed in (1, 2, 3)]
    assert all(_single(c[1]) for c in cases)
    if build == 'batch':
        cases = _batch_of(cases)
    for rule in ('bench', 'slack'):
        slots = [SLOT_RULES[rule](len(c[2])) for c in cases]
        assert _check_valid(cases, slots, _decode(cases, slots)) == len(cases)


def _overrun(kind):
    """a final metablock announcing MLEN = 4,096 whose commands produce more.  The writer sets
    MLEN from the commands; with lgwin 22 the header is 4 + 1 + 1 + 2 bits, so MLEN - 1 (4
    nibbles) is bytes 1 and 2 of the stream."""
    rng = random.Random(9)
    lits = lambda n: bytes(rng.choice(b'overun ') for _ in range(n))
    if kind == 'literals':    # the run that crosses 4,096 is literals
        cmds = [(lits(3000), 500, ('dist', 7)), (lits(2000), 2, None)]
    elif kind == 'copy':      # one copy from 3,000 to 5,000
        cmds = [(lits(3000), 2000, ('dist', 100)), (b'x', 2, None)]
    else:                     # a dictionary word that starts below 4,096 and ends beyond it
        cmds = [(lits(4090), 24, ('word', 5, 2)), (b'x', 2, None)]
    st = S.Stream(22, [S.MB('cmds', cmds=cmds)], 'overrun_' + kind)
    data = bytearray(S.build(st).data)
    assert (data[1] | data[2] << 8) + 1 > 4096
    data[1:3] = (4096 - 1).to_bytes(2, 'little')
    data = bytes(data)
    verdict = _oracle.decode(data, -1)   # (unknown-size mode, as a device call decodes)
    assert isinstance(verdict, int), 'the oracle accepts the overrunning stream'
    return ('overrun_' + kind, data, verdict)


@pytest.mark.parametrize('build', ['big', 'batch'])
def test_overrunning_streams_stay_in_their_slots(build):
    """Slots of 4,096 + slack between intact neighbours.  A literal run is cut at the announced
    total and goes on in the scratch ring (counted as left); a copy longer than the metablock's
    rest is refused before it stores, and a dictionary word ends inside the slack: those two end
    in the slot with the oracle's error, neither finished nor left."""
    good = [c for c in _valid() if c[4]][:4]
    bad = [_overrun(k) for k in ('literals', 'copy', 'word')]
    cases, slots, marks = [], [], []
    for k, b in enumerate(bad):
        cases += [good[k], b]
        slots += [len(good[k][2]) + SLACK, 4096 + SLACK]
        marks += [None, b]
    cases.append(good[3])
    slots.append(len(good[3][2]) + SLACK)
    marks.append(None)
    if build == 'batch':
        filler = _batch_of([c for c in _valid() if c[4]])
        cases += filler
        slots += [len(c[2]) + SLACK for c in filler]
        marks += [None] * len(filler)
    sizes, status, bufs, stats = _decode(cases, slots)
    ngood = 0
    for k, c in enumerate(cases):
        if marks[k] is None:
            assert status[k] == 0 and sizes[k] == len(c[2]) and bufs[k][:len(c[2])] == c[2], c[0]
            assert bufs[k][len(c[2]) + WORD_OVERSHOOT:] == bytes([SENT]) * (slots[k] - len(c[2]) - WORD_OVERSHOOT), c[0]
            ngood += 1
        else:
            assert status[k] == c[2], (c[0], status[k], c[2])
            # nothing at or beyond 4,096 + 36 of the slot
            assert bufs[k][4096 + WORD_OVERSHOOT:] == bytes([SENT]) * (SLACK - WORD_OVERSHOOT), c[0]
    assert stats == (ngood, 1), stats


@pytest.mark.parametrize('name', ['placed_12224', 'placed_90000'])
def test_damaged_streams(name):
    """the 40 truncations and 40 bit flips of an LDS-table and an HBM-table stream in slots of
    len(expected) + 4096 (the whole ring fits: kDirectRing) and of len(expected) + slack (by the
    announced total: kDirectSlot): the oracle's bytes or code for each"""
    exp_len = len(next(c[2] for c in _cases() if c[0] == name))
    # _corrupted's verdicts are brotliDecode's, which sizes its output from the header and stops
    # when it is full; a device call decodes in unknown-size mode to the stream's end (a
    # truncated stream whose bytes are all there is then -13): the oracle in that mode
    bad = [(n, d, _oracle.decode(d, -1)) for n, d, _ in _corrupted(name)]
    assert len(bad) == 80 and sum(1 for c in bad if isinstance(c[2], int)) >= 40
    for build, room in (('big', 4096), ('batch', 4096), ('big', SLACK), ('batch', SLACK)):
        cases = bad if build == 'big' else bad + _batch_of([c for c in _valid() if c[4]])
        assert (len(cases) <= _cus()) == (build == 'big')
        slots = [exp_len + room] * len(bad) + [len(c[2]) + room for c in cases[len(bad):]]
        sizes, status, bufs, stats = _decode(cases, slots)
        for k, (_, data, exp) in enumerate(bad):
            if isinstance(exp, int):
                assert status[k] == exp, (name, build, k, status[k], exp)
            else:
                assert status[k] == 0 and sizes[k] == len(exp) and bufs[k][:len(exp)] == exp, (name, build, k)
        for k in range(len(bad), len(cases)):
            c = cases[k]
            assert status[k] == 0 and bufs[k][:len(c[2])] == c[2], c[0]


def _not_eligible():
    rng = random.Random(3)
    out = []
    s = S.State(22)
    a = S.MB('cmds', cmds=S.gen_cmds(rng, s, 30, b'two metablocks '))
    b = S.MB('cmds', cmds=S.gen_cmds(rng, s, 30, b'second one.'))
    out.append(S.Stream(22, [a, b], 'two_metablocks'))
    out.append(S.long_run(100000, lgwin=16))          # the 64 KiB ring wraps
    out.append(S.Stream(22, [S.MB('raw', data=b'stored bytes ' * 40), S.MB('empty')], 'stored'))
    out.append(S.Stream(22, [S.MB('empty')], 'empty'))
    res = []
    for st in out:
        data = S.build(st).data
        res.append((st.name, data, S.model(st), st.lgwin, _single(data)))
        assert _oracle.decode(data) == res[-1][2]
    return res


@pytest.mark.parametrize('build', ['big', 'batch'])
def test_not_eligible(build):
    """two metablocks, a stored stream, the empty stream: through the scratch ring, whatever the
    slot.  A ring that must wrap: never by the announced total; where the slot holds the whole
    ring -- every slot that holds this stream does -- it begins in place, as it always did, and
    leaves at the wrap (_check_valid counts it as left)."""
    cases = _not_eligible()
    assert [c[4] for c in cases] == [False, True, False, False]   # (lgwin 16: one metablock, but larger than its ring)
    assert _ring(16, 100000) < 100000
    if build == 'batch':
        cases = _batch_of(cases)
    slots = [len(c[2]) + 4096 for c in cases]
    assert _check_valid(cases, slots, _decode(cases, slots)) == 0
    assert _in_place(16, 100000, 100000 + 4096, True) == 'left'
    slots = [len(c[2]) + SLACK for c in cases]
    assert _check_valid(cases, slots, _decode(cases, slots)) == 0
    assert _in_place(16, 100000, 100000 + SLACK, True) == 'left'   # (a slot that holds the stream holds its 64 KiB ring)


def test_custom_dictionary_stream():
    """brotliDecode with a customDictionary: never by the announced total (a compound copy that
    ends at the fence ends the call); the host call's power-of-two buffer holds the whole ring,
    so a one-metablock stream is in place by that rule"""
    from brotli_amd import datagen
    d = datagen.c5_dictionary()
    # the dictionary's tail where the window has nothing to offer: the stream start, and later
    data = d[-180:] + datagen.enwik_text(20000, 3) + d[-97:] + datagen.enwik_text(5000, 4)
    enc = brotli_amd.brotliEncode(data, {'quality': 11, 'lgwin': 22, 'customDictionary': d})
    assert _oracle.decode(enc, dictionary=d) == data
    refs0 = _oracle.compound_refs()
    _oracle.decode(enc, dictionary=d)
    assert _oracle.compound_refs() > refs0, 'the stream has no copy from the dictionary'
    assert brotli_amd.brotliDecode(enc, {'customDictionary': d}) == data
    alloc = 1
    while alloc < len(data):
        alloc <<= 1
    single = tuple(_oracle.trace(enc, dictionary=d)['metablocks']) == (1, 0, 0, 0)
    assert single and _ring(_lgwin(enc), len(data)) + 37 + 64 <= alloc + 4096
    assert brotli_amd.in_place_stats() == (1, 0)


def test_host_calls():
    """decode_batch pads its slots by the slack: the same bytes, every eligible stream in place;
    brotliDecode of each stream alone is unchanged"""
    cases = _valid()
    outs = brotli_amd.decode_batch([c[1] for c in cases])
    stats = brotli_amd.in_place_stats()
    for c, got in zip(cases, outs):
        assert got == c[2], c[0]
    assert stats == (sum(1 for c in cases if c[4]), 0), stats
    for c in cases:
        assert brotli_amd.brotliDecode(c[1]) == c[2], c[0]
        assert brotli_amd.in_place_stats() == (1 if c[4] else 0, 0), c[0]


def test_slack_constant_matches_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'brotli_amd.h')).read()
    assert int(re.search(r'#define\s+MIB_IN_PLACE_SLACK\s+(\d+)', src).group(1)) == SLACK
