"""A BrotliEncoder session with a prepared dictionary against the same session with the same
bytes as customDictionary (DESIGN.md 3d "Sessions"): encode rate and compressed size of one
session (quality 9, lgwin 22, 64 MiB fed in 1 MiB update() calls, five runs after a warm-up),
and the device memory that 64 encoder and 64 decoder sessions hold in either form.

    python scripts/dictionary_session_rate.py [--mib 64] [--dict-kib 1024] [--sessions 64] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
import brotli_amd  # noqa: E402
from brotli_amd import BrotliDecoder, BrotliEncoder, Dictionary  # noqa: E402


def document(r, n, D):
    """slices of D (40..300 bytes, from anywhere in it) and noise (20..200 bytes) in turn"""
    out, size = [], 0
    while size < n:
        k = r.randrange(40, 301)
        a = r.randrange(0, len(D) - k)
        out.append(D[a:a + k])
        out.append(r.randbytes(r.randrange(20, 201)))
        size += len(out[-2]) + len(out[-1])
    return b''.join(out)[:n]


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def encode(opts, doc, step):
    e = BrotliEncoder(opts)
    t0 = time.perf_counter()
    n = 0
    for at in range(0, len(doc), step):
        n += len(e.update(doc[at:at + step]))
    n += len(e.finish())
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=64)
    ap.add_argument('--dict-kib', type=int, default=1024)
    ap.add_argument('--sessions', type=int, default=64)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    r = random.Random(2025)
    D = r.randbytes(a.dict_kib << 10)
    doc = document(r, a.mib << 20, D)
    base = {'quality': 9, 'lgwin': 22}
    res = {'input_bytes': len(doc), 'dictionary_bytes': len(D), 'quality': 9, 'lgwin': 22, 'update_bytes': 1 << 20}
    with Dictionary(D) as handle:
        kinds = {'handle': dict(base, dictionary=handle), 'customDictionary': dict(base, customDictionary=D), 'none': dict(base)}
        for name, opts in kinds.items():
            encode(opts, doc, 1 << 20)   # warm-up
            runs = [encode(opts, doc, 1 << 20) for _ in range(a.runs)]
            secs = sorted(t for t, _ in runs)
            res[name] = {'compressed_bytes': runs[0][1], 'seconds': [round(t, 4) for t, _ in runs],
                         'median_MBps': round(len(doc) / secs[len(secs) // 2] / 1e6, 1)}
        # the sessions' device memory: every session has encoded / decoded one chunk
        small = doc[:1 << 20]
        streams = {}
        for name in ('handle', 'customDictionary'):
            e = BrotliEncoder(dict(kinds[name], quality=5))
            streams[name] = e.update(small) + e.finish()
        # (a first round, not recorded, grows the default context's workspaces to what the call needs)
        for name in ('handle', 'handle', 'customDictionary'):
            dec_opts = {'dictionary': handle} if name == 'handle' else {'customDictionary': D}
            before = free_bytes()
            es = [BrotliEncoder(dict(kinds[name], quality=5)) for _ in range(a.sessions)]
            ds = [BrotliDecoder(dict(dec_opts, outWindow=65536)) for _ in range(a.sessions)]
            brotli_amd.encoder_update_batch(es, [small[:200000]] * a.sessions)
            got = brotli_amd.decoder_update_batch(ds, [streams[name][:50000]] * a.sessions)
            assert all(isinstance(g, bytes) for g in got)
            held = before - free_bytes()
            res[name]['sessions'] = a.sessions
            res[name]['device_bytes_held_by_sessions'] = held
            del es, ds
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
