"""The measurements of DESIGN.md 4c "A batch of files": for k = 1, 8, 64 and 256 files, cycling
the five bench golden .woff2 files, the host wall time of woff2_decode_batch (min and max of five
calls after a warm-up) next to the same files through k woff2_decode calls in a loop; for k = 64
the device time of the batch's kernels (HIP events, default_profiling) and the share of the call
that the per-font glyf reconstruct loop takes (host wall time around the loop).  `--loop-only`
uses only the entry points that existed before woff2_decode_batch, so that the baseline can also
be taken on an older library (BROTLI_AMD_LIB).  One JSON line.
    python3 scripts/woff2_batch_timing.py [--loop-only] [--ks 1,8,64,256] [--calls 5]"""
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

PROFILED_K = 64


def timed(fn, calls):
    fn()   # warm-up
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return [round(min(out), 3), round(max(out), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loop-only', action='store_true')
    ap.add_argument('--ks', default='1,8,64,256')
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    bench = [fx[1] for fx in wf.golden_files() if fx[2] is None]
    assert len(bench) == 5
    out = {'library': os.path.basename(os.path.dirname(brotli_amd.library_path())), 'calls': a.calls, 'k': {}}
    for k in [int(v) for v in a.ks.split(',')]:
        files = [bench[i % len(bench)] for i in range(k)]
        row = {'woff2_bytes': sum(len(f) for f in files)}
        row['loop_ms_min_max'] = timed(lambda: [brotli_amd.woff2_decode(f) for f in files], a.calls)
        if not a.loop_only:
            row['batch_ms_min_max'] = timed(lambda: brotli_amd.woff2_decode_batch(files), a.calls)
            if k == PROFILED_K:
                # the unprofiled call's own split, then one profiled call for the device times
                brotli_amd.woff2_decode_batch(files)
                loop_ms, call_ms = brotli_amd.woff2_batch_last_ms()
                row['glyf_loop_ms'], row['call_ms'] = round(loop_ms, 3), round(call_ms, 3)
                row['glyf_loop_share'] = round(loop_ms / call_ms, 3)
                brotli_amd.default_profiling(True)
                brotli_amd.woff2_decode_batch(files)
                row['kernel_us_launches'] = {n: [round(v[0] * 1e3, 1), v[1]] for n, v in sorted(brotli_amd.default_kernel_times().items())}
                brotli_amd.default_profiling(False)
        out['k'][str(k)] = row
    print(json.dumps(out))


if __name__ == '__main__':
    main()
