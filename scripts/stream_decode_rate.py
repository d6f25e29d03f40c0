"""Streaming decode rate: one C4-style 1 MiB stream and one 64 MiB single stream through
BrotliDecoder at 64 KiB, 1 MiB and 16 MiB updates, and through brotliDecode (mib_decode) in the
same run; MB/s of output, the ratio to one-shot, device passes and re-decoded output bytes per
update.  One JSON line.

    python scripts/stream_decode_rate.py [--reps 3] [--quality 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--quality', type=int, default=5)
    a = ap.parse_args()
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
