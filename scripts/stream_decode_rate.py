"""Streaming decode rate: one C4-style 1 MiB stream and one 64 MiB single stream through
BrotliDecoder at 64 KiB, 1 MiB and 16 MiB updates, and through brotliDecode (mib_decode) in the
same run; MB/s of output, the ratio to one-shot, device passes and re-decoded output bytes per
update.  One JSON line.

    python scripts/stream_decode_rate.py [--reps 3] [--quality 5]

--sessions K: K sessions, each decoding its own 1 MiB stream (a seed per session) in 64 KiB
updates, all through decoder_update_batch, and in the same process the same sessions one after
another through update(); aggregate MB/s of both, the batch's launches and rounds, and one
round's host wall time by phase.

    python scripts/stream_decode_rate.py --sessions 64 [--out-window 65536] [--solo-cap 64]

--device (with --sessions): the same sessions and updates through decoder_update_batch_device as
well, chunks and output in torch tensors, interleaved with the host batch in the same process;
adds a "device" entry with its MB/s, launches and a round's phases (the download leg stays 0).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
import brotli_amd   # noqa: E402
from brotli_amd import datagen   # noqa: E402


def best(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), r


def stream(comp, chunk):
    d = brotli_amd.BrotliDecoder()
    n, updates = 0, 0
    for at in range(0, len(comp), chunk):
        n += len(d.update(comp[at:at + chunk]))
        updates += 1
    n += len(d.finish())
    return n, updates, d.passes, d.redecoded


def _text(seed):
    return bytes(datagen.enwik_text(1 << 20, seed))


def _batch_counters():
    import ctypes
    lib = brotli_amd._L()
    n = ctypes.c_uint64()
    ms = (ctypes.c_double * 5)()
    lib.mib_decoder_batch_stats(ctypes.byref(n))
    lib.mib_decoder_batch_times(ms, 5)
    return int(n.value), list(ms)


def sessions(a):
    """K sessions, each its own 1 MiB stream (seed 5 + i), in 64 KiB updates: all of them
    through decoder_update_batch, and (the first --solo-cap of them) one after another through
    update(): the same rounds, a session per call."""
    k, chunk = a.sessions, 64 << 10
    opts = {'outWindow': a.out_window} if a.out_window else None
    # (worker processes make the texts before this process opens the GPU; they never open it)
    import multiprocessing
    with multiprocessing.get_context('fork').Pool(min(16, k)) as pool:
        plains = pool.map(_text, range(5, 5 + k))
    comps = []
    for at in range(0, k, 64):
        comps += brotli_amd.encode_batch(plains[at:at + 64], {'quality': a.quality})
    total = sum(len(p) for p in plains)
    steps = max((len(c) + chunk - 1) // chunk for c in comps)

    def run_batch():
        ds = [brotli_amd.BrotliDecoder(opts) for _ in comps]
        n0, ms0 = _batch_counters()
        t0 = time.perf_counter()
        outs = [[] for _ in comps]
        for t in range(steps):
            res = brotli_amd.decoder_update_batch(ds, [c[t * chunk:(t + 1) * chunk] for c in comps])
            for i, r in enumerate(res):
                outs[i].append(r)
        for i, r in enumerate(brotli_amd.decoder_finish_batch(ds)):
            outs[i].append(r)
        dt = time.perf_counter() - t0
        n1, ms1 = _batch_counters()
        return dt, outs, n1 - n0, [b - x for x, b in zip(ms0, ms1)], max(d.passes for d in ds)

    def run_solo(m):
        ds = [brotli_amd.BrotliDecoder(opts) for _ in range(m)]
        t0 = time.perf_counter()
        outs = []
        for d, c in zip(ds, comps):
            got = [d.update(c[at:at + chunk]) for at in range(0, len(c), chunk)]
            got.append(d.finish())
            outs.append(got)
        return time.perf_counter() - t0, outs

    if a.device:
        # the chunks resident in HBM, step by step back to back (a call's chunks are one run of
        # d_in); every call writes into the same k ranges of `room` bytes, which hold a whole
        # stream, so no slot ever reports MORE_OUTPUT
        import torch
        room = 1 << 20
        step_at, flat = [], bytearray()
        for t in range(steps):
            offs = [len(flat)]
            for c in comps:
                flat += c[t * chunk:(t + 1) * chunk]
                offs.append(len(flat))
            step_at.append(offs)
        d_in = torch.frombuffer(flat, dtype=torch.uint8).to('cuda')
        d_out = torch.empty(k * room, dtype=torch.uint8, device='cuda')
        out_offs = [i * room for i in range(k + 1)]
        torch.cuda.synchronize()

    def run_device(verify):
        """the same sessions and updates through the device calls; verify: every call's bytes are
        fetched and returned (not a timed run)"""
        ds = [brotli_amd.BrotliDecoder(opts) for _ in comps]
        n0, ms0 = _batch_counters()
        t0 = time.perf_counter()
        outs = [[] for _ in comps]
        total_out = 0
        for t in range(steps + 1):
            if t < steps:
                sizes, st = brotli_amd.decoder_update_batch_device(ds, d_in.data_ptr(), step_at[t], d_out.data_ptr(), out_offs)
            else:
                sizes, st = brotli_amd.decoder_finish_batch_device(ds, d_out.data_ptr(), out_offs)
            assert not any(st), st
            total_out += sum(sizes)
            if verify:
                for i, n in enumerate(sizes):
                    outs[i].append(d_out[i * room:i * room + n].cpu().numpy().tobytes())
        dt = time.perf_counter() - t0
        n1, ms1 = _batch_counters()
        assert total_out == total
        return dt, outs, n1 - n0, [b - x for x, b in zip(ms0, ms1)], max(d.passes for d in ds)

    best_b = best_s = best_d = None
    m = min(k, a.solo_cap) if a.solo_cap else k
    if a.device:
        rd = run_device(True)
        assert all(b''.join(o) == p for o, p in zip(rd[1], plains))
    for _ in range(a.reps):   # interleaved: batch, (device,) solo, batch, (device,) solo
        rb = run_batch()
        assert all(b''.join(o) == p for o, p in zip(rb[1], plains))
        rb = (rb[0], None) + rb[2:]
        best_b = rb if best_b is None or rb[0] < best_b[0] else best_b
        if a.device:
            rd = run_device(False)
            best_d = rd if best_d is None or rd[0] < best_d[0] else best_d
        ts, so = run_solo(m)
        assert all(b''.join(o) == p for o, p in zip(so, plains))
        best_s = ts if best_s is None or ts < best_s else best_s
    dt, _, launches, ms, rounds = best_b
    solo_rate = sum(len(p) for p in plains[:m]) / best_s / 1e6
    names = ('upload_ms', 'launch_ms', 'readback_ms', 'delivery_ms', 'download_ms')
    res = {'sessions': k, 'quality': a.quality, 'update_bytes': chunk, 'out_window': a.out_window or (16 << 20),
           'updates_per_session': steps, 'batch_MBps': round(total / dt / 1e6, 1),
           'solo_sessions_timed': m, 'one_after_another_MBps': round(solo_rate, 2),
           'speedup': round(total / dt / 1e6 / solo_rate, 1), 'launches': launches,
           'neediest_session_passes': rounds, 'batch_seconds': round(dt, 4),
           'per_round': {nm: round(v / max(1, launches), 3) for nm, v in zip(names, ms)},
           'host_outside_rounds_ms_per_call': round((1e3 * dt - sum(ms)) / (steps + 1), 3)}
    if a.device:
        ddt, _, dlaunches, dms, drounds = best_d
        res['device'] = {'MBps': round(total / ddt / 1e6, 1), 'against_batch': round(dt / ddt, 3), 'launches': dlaunches,
                         'neediest_session_passes': drounds, 'seconds': round(ddt, 4),
                         'per_round': {nm: round(v / max(1, dlaunches), 3) for nm, v in zip(names, dms)},
                         'host_outside_rounds_ms_per_call': round((1e3 * ddt - sum(dms)) / (steps + 1), 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--quality', type=int, default=5)
    ap.add_argument('--sessions', type=int, default=0,
                    help='K sessions through decoder_update_batch against the same sessions one after another')
    ap.add_argument('--out-window', type=int, default=0, help='outWindow of the sessions (0: the default, 16 MiB)')
    ap.add_argument('--solo-cap', type=int, default=0,
                    help='time at most this many of the K sessions one after another (0: all of them)')
    ap.add_argument('--device', action='store_true',
                    help='with --sessions: the same sessions and updates through decoder_update_batch_device too '
                         '(chunks and output in torch tensors), interleaved with the host batch')
    a = ap.parse_args()
    if a.sessions:
        return sessions(a)
    res = {'quality': a.quality, 'cases': []}
    for name, size in (('c4_1MiB', 1 << 20), ('c2_64MiB', 64 << 20)):
        plain = bytes(datagen.enwik_text(size, 5))
        comp = brotli_amd.brotliEncode(plain, {'quality': a.quality})
        assert brotli_amd.brotliDecode(comp) == plain
        t1, _ = best(lambda: brotli_amd.brotliDecode(comp), a.reps)
        one = len(plain) / t1 / 1e6
        for chunk in (64 << 10, 1 << 20, 16 << 20):
            t, (n, updates, passes, redone) = best(lambda: stream(comp, chunk), a.reps)
            assert n == len(plain)
            res['cases'].append({'stream': name, 'compressed': len(comp), 'update_bytes': chunk, 'updates': updates,
                                 'passes': passes, 'passes_per_update': round(passes / updates, 2),
                                 'redecoded_bytes': redone, 'redecoded_per_update': round(redone / updates, 1),
                                 'stream_MBps': round(len(plain) / t / 1e6, 1), 'oneshot_MBps': round(one, 1),
                                 'ratio': round(len(plain) / t / 1e6 / one, 4)})
    print(json.dumps(res))


if __name__ == '__main__':
    main()
