"""Device-resident batches of streaming decoder sessions (decoder_update_batch_device /
decoder_finish_batch_device, DESIGN.md §4d "Device-resident batches"): the chunks are read from
and the decoded bytes written to device memory (torch tensors here).

Expected bytes and codes are the oracle's (tests/_oracle.py) and the stream model's
(tests/_streams.py), shared with tests/test_gpu_stream_decode_batch.py (its corpus and its
cached oracle results); "equals host" compares with host BrotliDecoder sessions fed the same
chunks.  Nothing expected comes from the device path.

Ranges are laid back to back from an odd offset, as the offset arrays of the call have them: a
slot that wrote behind its range would damage its neighbour's bytes, which are compared, and the
canaries in front of the first and behind the last range must stay."""
import base64
import json
import os
import random
import re

import numpy as np
import pytest

import _oracle
import _streams as S
import brotli_amd
import test_gpu_stream_decode_batch as B

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

MORE = brotli_amd.MORE_OUTPUT
CANARY = 0xA5
PAD = 77   # the first range starts at this (odd) offset; as many canary bytes behind the last
WIN = B.WIN

_cache = {}


def _raw_200k():
    """one uncompressed metablock of 200,000 bytes: a single launch yields all of it, however
    small the room (an uncompressed metablock is one command)"""
    if 'raw' not in _cache:
        data = random.Random(5).randbytes(200000)
        st = S.Stream(18, [S.MB('raw', data=data), S.MB('empty')], 'raw_200k')
        enc = S.build(st).data
        assert _oracle.decode(enc, -1) == data == S.model(st)
        _cache['raw'] = ('raw_200k', enc, data)
    return _cache['raw']


def _corpus():
    return B._streams() + [_raw_200k()]


class _Out:
    """the callers' ranges: rooms[i] bytes per slot, back to back from PAD, canaries around"""

    def __init__(self, rooms):
        self.rooms = list(rooms)
        self.off = [PAD]
        for r in self.rooms:
            self.off.append(self.off[-1] + r)
        self.t = torch.full((self.off[-1] + PAD,), CANARY, dtype=torch.uint8, device='cuda')

    def ptr(self):
        return self.t.data_ptr()

    def take(self, sizes):
        parts = [self.t[o:o + n] for o, n in zip(self.off, sizes) if n]
        flat = torch.cat(parts).cpu().numpy().tobytes() if parts else b''
        out, at = [], 0
        for n in sizes:
            out.append(flat[at:at + n])
            at += n
        return out

    def intact(self):
        ends = torch.cat([self.t[:PAD], self.t[self.off[-1]:]]).cpu().numpy()
        return bool((ends == CANARY).all())


def _call(ds, chunks, out, finish=False):
    """one device call; returns (per slot bytes, statuses) after the contract's checks"""
    if finish:
        sizes, st = brotli_amd.decoder_finish_batch_device(ds, out.ptr(), out.off)
    else:
        buf = bytearray(b'\xee' * 3 + b''.join(chunks))   # chunks back to back from offset 3
        offs = [3]
        for c in chunks:
            offs.append(offs[-1] + len(c))
        d_in = torch.frombuffer(buf, dtype=torch.uint8).to('cuda')
        torch.cuda.synchronize()   # the caller's writes are complete before the call
        sizes, st = brotli_amd.decoder_update_batch_device(ds, d_in.data_ptr(), offs, out.ptr(), out.off)
    assert out.intact(), 'a byte outside the ranges was written'
    for i, (n, s) in enumerate(zip(sizes, st)):
        if s == MORE:
            assert n == out.rooms[i], (i, n, out.rooms[i])
        elif s == 0:
            assert n <= out.rooms[i], (i, n, out.rooms[i])
        else:
            assert s < 0 and (n == 0 or s == -103), (i, n, s)
    return out.take([n if s >= 0 else 0 for n, s in zip(sizes, st)]), st, sizes


def _run(items, rooms, drain, expected=()):
    """items: [(data, sizes, opts)] in lock step through the device calls (expected: the streams'
    outputs, which bound the number of draining calls).  Per session a list
    with each step's (status, bytes) -- with `drain`, a step is the call and the calls with empty
    chunks that follow until no slot reports MORE_OUTPUT, its bytes joined -- then finished, then
    the finish step's (status, bytes); and the most bytes any session was seen holding."""
    steps = max(len(sizes) for _, sizes, _ in items)
    feeds = [B._chunks(data, sizes, steps) for data, sizes, _ in items]
    ds = [brotli_amd.BrotliDecoder(opts) for _, _, opts in items]
    out = _Out(rooms)
    k = len(ds)
    most_held = 0

    def step(chunks, finish):
        nonlocal most_held
        got, st, _ = _call(ds, chunks, out, finish)
        most_held = max([most_held] + [d.held_output for d in ds])
        calls = 0
        while drain and MORE in st:
            # (a full range hands out `room` bytes a call; a few calls more for launches that add nothing)
            calls += 1
            assert calls <= max(len(data) for data in expected) // max(1, min(out.rooms)) + 8, 'the drain does not end'
            more, st2, _ = _call(ds, [b''] * k, out, finish)
            most_held = max([most_held] + [d.held_output for d in ds])
            for i in range(k):
                if st[i] == MORE:
                    got[i] += more[i]
                    st[i] = st2[i]
                else:
                    assert st2[i] == st[i] and more[i] == b'', i   # nothing more, or the same error again
        return list(zip(st, got))

    res = [[] for _ in items]
    for t in range(steps):
        for i, r in enumerate(step([f[t] for f in feeds], False)):
            res[i].append(r)
    fin = [d.finished for d in ds]
    tails = step(None, True)
    return ds, feeds, res, fin, tails, most_held


def _host_key(r):
    """a host call's result as the device call reports it: (status, bytes)"""
    return (r.code, b'') if isinstance(r, brotli_amd.BrotliError) else (0, r)


def _assert_equals_host(cs, items):
    """the device run with 2 MiB of room per slot against host sessions fed the same chunks, call
    by call; and the decode launches of both runs"""
    before = B._batch_launches()
    ds, feeds, res, fin, tails, most_held = _run(items, [2 << 20] * len(items), drain=False)
    made = B._batch_launches() - before
    before = B._batch_launches()
    hs, hfeeds, hres, hfin, htails = B._batch(items)
    host_made = B._batch_launches() - before
    assert most_held == 0   # ample room: nothing is ever left behind
    for i, (nm, _, exp) in enumerate(cs):
        assert feeds[i] == hfeeds[i]
        assert res[i] == [_host_key(r) for r in hres[i]], nm
        assert tails[i] == _host_key(htails[i]) and fin[i] == hfin[i], nm
        assert (ds[i].finished, ds[i].passes, ds[i].redecoded) == (hs[i].finished, hs[i].passes, hs[i].redecoded), nm
        assert b''.join(b for _, b in res[i]) == exp and fin[i] is True and tails[i] == (0, b''), nm
    print('decode launches: device %d, host %d' % (made, host_made))
    assert made == host_made


# ---------------------------------------------------------------- 1. the copy kernel alone
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097)


def test_copy_kernel_alignments_and_edges():
    """every (src & 15, dst & 15) pair at every length around a granule and a tile, one copy of
    more tiles than a descriptor gets blocks, and destinations that abut inside one granule: one
    launch; the copied bytes are the sources, every other byte of the destination buffer is canary"""
    copies = []   # (src offset, dst offset, n)
    sat = dat = 16
    for sa in range(16):
        for da in range(16):
            for n in LENGTHS:
                copies.append((sat + sa, dat + da, n))
                sat += (sa + n + 47) & ~15
                dat += (da + n + 47) & ~15
    copies.append((sat + 3, dat + 9, (1 << 20) + 17))
    assert ((1 << 20) + 17 + 9 + 4095) // 4096 > 256   # more tiles than kGatherSpread blocks
    sat += (1 << 20) + 64
    dat += (1 << 20) + 64
    for a, n1, n2 in ((0, 5, 7), (3, 1, 1), (9, 17, 3), (15, 4095, 18), (6, 2, 4097), (1, 14, 1), (0, 16, 5)):
        # the second destination starts where the first ends, inside one 16-byte granule (or, for
        # the last pair, on its boundary)
        copies.append((sat + 11, dat + a, n1))
        copies.append((sat + 11 + n1 + 5, dat + a + n1, n2))
        if n1 != 16:
            assert (dat + a + n1 - 1) // 16 == (dat + a + n1) // 16
        sat += n1 + n2 + 64
        dat += (a + n1 + n2 + 47) & ~15
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, sat + 64, dtype=np.uint8)
    want = np.full(dat + 64, CANARY, dtype=np.uint8)
    for s, d, n in copies:
        assert (want[d:d + n] == CANARY).all()   # (the destinations are disjoint)
        want[d:d + n] = src[s:s + n]
    d_src = torch.from_numpy(src).to('cuda')
    d_dst = torch.full((dat + 64,), CANARY, dtype=torch.uint8, device='cuda')
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    seen = {((d_src.data_ptr() + s) & 15, (d_dst.data_ptr() + d) & 15) for s, d, _ in copies}
    assert len(seen) == 256
    torch.cuda.synchronize()
    assert len(copies) < 65535   # one launch
    brotli_amd.debug_copy_batch([d_src.data_ptr() + s for s, _, _ in copies], [d_dst.data_ptr() + d for _, d, _ in copies],
                                [n for _, _, n in copies])
    got = d_dst.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- 2. equals host, ample room
def test_equals_host_with_ample_room():
    """the whole corpus as one batch in lock-step 4,096-byte chunks, odd offsets, 2 MiB a slot"""
    cs = _corpus()
    _assert_equals_host(cs, [(data, B._cuts_fixed(len(data), 4096), None) for _, data, _ in cs])


# ---------------------------------------------------------------- 3. tight room
# Room 1 hands out one byte a call, so a stream takes as many calls as it has output bytes: it
# runs on the streams of up to 2 KiB of output, the other rooms on every stream.
@pytest.mark.parametrize('room', [1, 4097, 65536])
def test_tight_room(room):
    cs = [c for c in _corpus() if room > 1 or len(c[2]) <= 2048]
    assert len(cs) >= 20
    items = [(data, B._cuts_fixed(len(data), 4096), {'outWindow': WIN}) for _, data, _ in cs]
    ds, feeds, res, fin, tails, most_held = _run(items, [room] * len(items), drain=True, expected=[c[2] for c in cs])
    for i, (nm, _, exp) in enumerate(cs):
        assert all(s == 0 for s, _ in res[i]) and tails[i][0] == 0, nm
        assert b''.join(b for _, b in res[i]) + tails[i][1] == exp, nm
        assert fin[i] is True and ds[i].finished and ds[i].held_output == 0, nm
    print('room %d: most bytes held by a session %d' % (room, most_held))
    if room > 1:
        # raw_200k's one launch yields 200,000 bytes whatever the room: the held path is taken
        assert most_held >= 200000 - room >= (64 << 10)


# ---------------------------------------------------------------- 4. room 0
def test_room_zero_makes_no_launch():
    nm, data, exp = B._by_name('alice29.txt.compressed')
    d = brotli_amd.BrotliDecoder()
    before = B._batch_launches()
    got, st, sizes = _call([d], [data], _Out([0]))
    assert (st, sizes, got) == ([MORE], [0], [b'']) and d.passes == 0 and B._batch_launches() == before
    assert d.held_output == 0 and not d.finished   # (the launch is owed, nothing is decoded)
    got, st, sizes = _call([d], [b''], _Out([0]))   # ... again
    assert (st, sizes) == ([MORE], [0]) and d.passes == 0
    got, st, sizes = _call([d], [b''], _Out([len(exp) + 5]))
    assert st == [0] and got == [exp] and d.passes == 1 and d.finished
    # a session that holds bytes: room 0 hands out nothing and launches nothing
    nm, data, exp = _raw_200k()
    d = brotli_amd.BrotliDecoder()
    got, st, _ = _call([d], [data], _Out([10]))
    assert st == [MORE] and got == [exp[:10]] and d.held_output == len(exp) - 10 and d.passes == 1
    got, st, sizes = _call([d], [b''], _Out([0]))
    assert (st, sizes) == ([MORE], [0]) and d.passes == 1 and d.held_output == len(exp) - 10
    got, st, _ = _call([d], [b''], _Out([len(exp)]))
    assert st == [0] and got == [exp[10:]] and d.held_output == 0 and d.finished


# ---------------------------------------------------------------- 5. mixed calls
def test_mixed_device_and_host_calls():
    """each session's chunks go through a device call (a small room) or a host update() by seeded
    choice; held bytes come out of whichever call is next, a host update(b'') and a host
    finish() on a finished session included"""
    names = ('alice29.txt.compressed', 'mapsdatazrh.compressed', 'zeros.compressed', 'transitions', 'ring_wrap')
    cs = [B._by_name(n) for n in names] + [_raw_200k()]
    rng = random.Random(23)
    picked_up = 0
    for nm, data, exp in cs:
        d = brotli_amd.BrotliDecoder({'outWindow': WIN})
        got = []
        for piece in B._chunks(data, B._cuts_fixed(len(data), 3000), 0):
            if rng.random() < 0.5:
                b, st, _ = _call([d], [piece], _Out([rng.choice([0, 1, 100, 5000, 70000])]))
                assert st[0] in (0, MORE), nm
                got.append(b[0])
                if st[0] == MORE and rng.random() < 0.5:
                    held = d.held_output
                    more = d.update(b'')   # the host call returns what is held, then goes on
                    assert len(more) >= held and d.held_output == 0, nm
                    picked_up += held > 0
                    got.append(more)
            else:
                got.append(d.update(piece))
                assert d.held_output == 0, nm
        got.append(d.finish())
        assert b''.join(got) == exp and d.finished and d.held_output == 0, nm
    assert picked_up >= 3
    # a session that holds bytes and owes a launch (the raw metablock came whole, the last, empty
    # metablock is still to be read): host finish() returns the rest; so does update(b'')
    nm, data, exp = _raw_200k()
    for last in ('finish', 'update'):
        d = brotli_amd.BrotliDecoder()
        b, st, _ = _call([d], [data], _Out([10]))
        assert st == [MORE] and d.held_output == len(exp) - 10
        rest = d.finish() if last == 'finish' else d.update(b'')
        assert b[0] + rest == exp and d.held_output == 0 and d.finished
        assert d.finish() == b''
    # ... in batch calls too, beside a session driven by host calls alone
    d, other = brotli_amd.BrotliDecoder(), brotli_amd.BrotliDecoder()
    b, st, _ = _call([d], [data], _Out([10]))
    r = brotli_amd.decoder_update_batch([d, other], [b'', data])
    assert b[0] + r[0] == exp and r[1] == exp
    assert brotli_amd.decoder_finish_batch([d, other]) == [b'', b'']
    # (A session that reports finished never holds bytes: a launch meets a boundary behind the
    # stream's last command too, where it leaves on the output limit before it reports the end.
    # So the end is always reported by a launch that stayed below its limit, whose bytes fit.)
    # finish() on a finished session with nothing held is what it was: nothing
    assert d.finished and d.held_output == 0 and d.finish() == b'' and d.update(b'') == b''

# ---------------------------------------------------------------- 6. errors per slot
def _host_outcome(data, opts=None):
    """(code, total in the limit's message or None) of a host session given the stream whole"""
    _, res, _, tail = B._solo([data], opts)
    for r in res + [tail]:
        if isinstance(r, brotli_amd.BrotliError):
            m = re.match(r'Decompressed size (\d+) exceeds', str(r))
            return r.code, int(m.group(1)) if m else None
    return 0, None


def test_errors_are_per_slot():
    with open(os.path.join(B.G, 'decode_errors.json')) as f:
        cases = json.load(f)['cases']
    bad = [base64.b64decode(c['in_b64']) for c in cases[5::101]]
    assert len(bad) >= 6
    _, valid, valid_exp = B._by_name('alice29.txt.compressed')
    _, small, _ = B._by_name('10x10y.compressed')
    streams = bad + [valid, small + b'\x01\x02\x03', valid, valid]
    opts = [None] * (len(bad) + 2) + [{'maxOutputSize': len(valid_exp) - 1}, {'maxOutputSize': len(valid_exp)}]
    want = [_host_outcome(s, o) for s, o in zip(streams, opts)]
    assert sum(1 for c, _ in want[:len(bad)] if c < 0) >= 5
    assert want[len(bad):] == [(0, None), (-17, None), (-103, len(valid_exp)), (0, None)]
    for s, (c, _) in zip(bad, want):
        ora = _oracle.decode(s, -1)
        assert c == (ora if isinstance(ora, int) else 0)
    ds = [brotli_amd.BrotliDecoder(o) for o in opts]
    out = _Out([1 << 20] * len(ds))
    got, st1, sz1 = _call(ds, streams, out)
    tails, st2, sz2 = _call(ds, None, out, finish=True)
    again, st3, sz3 = _call(ds, [b''] * len(ds), out)
    for i, (code, total) in enumerate(want):
        first = st1[i] if st1[i] < 0 else st2[i]
        assert first == code, (i, st1[i], st2[i], code)
        if code == 0:
            assert got[i] + tails[i] == _oracle.decode(streams[i], -1) and ds[i].finished, i
            if streams[i] is valid:
                assert got[i] == valid_exp   # the neighbours' errors did not reach it
            assert st3[i] == 0 and sz3[i] == 0
            continue
        size = sz1[i] if st1[i] < 0 else sz2[i]
        assert size == (total if code == -103 else 0), (i, size)
        # sticky: every later call reports the code again
        assert st3[i] == code and (st1[i] == code or st1[i] == 0) and st2[i] == code, i
        assert ds[i].held_output == 0
        try:
            ds[i].update(b'')
            raise AssertionError('the failed session took a host call')
        except brotli_amd.BrotliError as e:
            assert e.code == code


# ---------------------------------------------------------------- 7. both LDS builds
def test_equals_host_in_the_four_per_cu_build():
    names = {st.name for st in S.named()}
    cs = [c for c in B._streams() if c[0] in names]
    assert len(cs) >= 12
    lib = brotli_amd._L()
    try:
        lib.mib_force_decoder_build(1)
        _assert_equals_host(cs, [(data, B._cuts_fixed(len(data), 4096), None) for _, data, _ in cs])
    finally:
        lib.mib_force_decoder_build(0)
