"""The measurements of DESIGN.md 4c "Writing a file": for k = 1, 8 and 64 fonts, cycling the three
bench source fonts (enc-ttf, enc-var-ttf, enc-otf), the host wall time of woff2_encode_batch (min
and max of five calls after a warm-up) next to the route a caller had before it: per font
woff2_transform_glyf, woff2_transform_hmtx and brotliEncode (FONT mode, quality 11) with the
container written in Python (tests/_woff2_file.write).  For k = 64 the device time of the batch's
kernels (HIP events, default_profiling).  `--loop-only` uses only the entry points that existed
before woff2_encode, so that the baseline can be taken on an older library (BROTLI_AMD_LIB).
`--batch-only` times woff2_encode_batch alone (the rows that are re-measured against a parent
library).  `--collection` adds the row of DESIGN.md 4c "Writing a collection": the two-member
collection over enc-ttf (the source font of enc-ttf-hmtx; the members share every table but name)
as one woff2_encode call, against woff2_encode_batch over its two members as single fonts -- what
a caller could do before --, time and bytes; and the same collection with every table written
twice (nothing shared by offset), whose call holds the compare launch (`w2enc_same`).
One JSON line.
    python3 scripts/woff2_encode_timing.py [--loop-only] [--batch-only] [--collection] [--ks 1,8,64] [--calls 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import brotli_amd  # noqa: E402
import _woff2_file as wf  # noqa: E402
import _woff2_write as ww  # noqa: E402

PROFILED_K = 64


def timed(fn, calls):
    fn()   # warm-up
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return [round(min(out), 3), round(max(out), 3)]


def by_hand(font):
    """the file of one font, the way tests/_woff2_file.product_file writes it: two transform calls
    (an upload of the font's tables each), an encode call, the container in Python"""
    t = wf.sfnt_tables(font)
    parts = {}
    if b'glyf' in t:
        parts[b'glyf'], parts[b'loca'] = brotli_amd.woff2_transform_glyf(font), b''
        thmtx = brotli_amd.woff2_transform_hmtx(font)
        if thmtx is not None:
            parts[b'hmtx'] = thmtx
    stream, entries = b'', []
    for tag in sorted(t):
        if tag == b'DSIG':
            continue
        if tag in parts:
            entries.append([tag, 1 if tag == b'hmtx' else 0, len(t[tag]), len(parts[tag])])
            stream += parts[tag]
        else:
            data = t[tag]
            if tag == b'head':
                data = data[:8] + bytes(4) + data[12:16] + bytes([data[16] | (8 if parts else 0)]) + data[17:]
            entries.append([tag, 0, len(data), None])
            stream += data
    comp = brotli_amd.brotliEncode(stream, {'quality': 11, 'lgwin': 22, 'mode': brotli_amd.EncoderMode.FONT})
    return wf.write(int.from_bytes(font[:4], 'big'), entries, comp)


def collection_row(calls):
    import _woff2_collection as wc
    import _woff2_collection_write as cw
    t = wf.sfnt_tables(ww._source('enc-ttf'))
    name2 = bytes([t[b'name'][0]]) + t[b'name'][1:-1] + bytes([t[b'name'][-1] ^ 1])
    a = sorted(t.items())
    b = [(tag, name2 if tag == b'name' else data) for tag, data in a]
    row = {}
    for key, share in (('shared', True), ('unshared', False)):
        ttc = cw.build_ttc(wc.V1, [(wc.V1, a), (wc.V1, b)], share=share)
        members = [cw.member_sfnt(ttc, 0), cw.member_sfnt(ttc, 1)]
        r = {'ttc_bytes': len(ttc), 'member_bytes': sum(len(m) for m in members), 'candidates': len(cw.candidates(ttc))}
        r['collection_ms_min_max'] = timed(lambda: brotli_amd.woff2_encode(ttc), calls)
        r['members_batch_ms_min_max'] = timed(lambda: brotli_amd.woff2_encode_batch(members), calls)
        file = brotli_amd.woff2_encode(ttc)
        r['collection_woff2_bytes'] = len(file)
        r['directory_entries'] = int.from_bytes(file[12:14], 'big')
        r['members_woff2_bytes'] = sum(len(f) for f in brotli_amd.woff2_encode_batch(members))
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_encode(ttc)
        r['kernel_us_launches'] = {n: [round(v[0] * 1e3, 1), v[1]] for n, v in sorted(brotli_amd.default_kernel_times().items())
                                   if n.startswith('w2enc')}
        brotli_amd.default_profiling(False)
        row[key] = r
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loop-only', action='store_true')
    ap.add_argument('--batch-only', action='store_true')
    ap.add_argument('--collection', action='store_true')
    ap.add_argument('--ks', default='1,8,64')
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    bench = [ww._source(name) for name in ('enc-ttf', 'enc-var-ttf', 'enc-otf')]
    out = {'library': os.path.basename(os.path.dirname(brotli_amd.library_path())), 'calls': a.calls, 'k': {}}
    for k in [int(v) for v in a.ks.split(',')]:
        fonts = [bench[i % len(bench)] for i in range(k)]
        row = {'sfnt_bytes': sum(len(f) for f in fonts)}
        if a.batch_only:
            row['batch_ms_min_max'] = timed(lambda: brotli_amd.woff2_encode_batch(fonts), a.calls)
            row['batch_woff2_bytes'] = sum(len(f) for f in brotli_amd.woff2_encode_batch(fonts))
            out['k'][str(k)] = row
            continue
        row['loop_ms_min_max'] = timed(lambda: [by_hand(f) for f in fonts], a.calls)
        row['loop_woff2_bytes'] = sum(len(by_hand(f)) for f in fonts)
        if not a.loop_only:
            row['batch_ms_min_max'] = timed(lambda: brotli_amd.woff2_encode_batch(fonts), a.calls)
            files = brotli_amd.woff2_encode_batch(fonts)
            row['batch_woff2_bytes'] = sum(len(f) for f in files)
            row['solo_loop_ms_min_max'] = timed(lambda: [brotli_amd.woff2_encode(f) for f in fonts], a.calls)
            if k == PROFILED_K:
                brotli_amd.default_profiling(True)
                brotli_amd.woff2_encode_batch(fonts)
                row['kernel_us_launches'] = {n: [round(v[0] * 1e3, 1), v[1]] for n, v in sorted(brotli_amd.default_kernel_times().items())}
                brotli_amd.default_profiling(False)
        out['k'][str(k)] = row
    if a.collection:
        out['collection'] = collection_row(a.calls)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
