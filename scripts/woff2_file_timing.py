"""The measurements of DESIGN.md 4c "A whole file": on a golden .woff2 file (default
enc-ttf-hmtx), the device time of woff2_decode's kernels (HIP events, default_profiling), the
host wall time of woff2_decode over five calls after a warm-up, and -- `--sequence`, which uses
only the entry points that existed before woff2_decode, so that it also runs on an older
library (BROTLI_AMD_LIB) -- the wall time of what a caller had to do instead: brotliDecode,
cutting the tables on the host, woff2_reconstruct_glyf, woff2_reconstruct_hmtx (no assembly, no
checksums).  One JSON line.
    python3 scripts/woff2_file_timing.py [--file NAME] [--sequence]"""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import brotli_amd  # noqa: E402
import _woff2_file as wf  # noqa: E402


def timed(fn, calls=5):
    fn()   # warm-up
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return [round(min(out), 3), round(max(out), 3)]


def sequence(data):
    """what a caller of the older library does with a .woff2 file's tables"""
    _, ent, comp = wf.parse(data)
    state = {e[0]: wf.is_transformed(e[0], e[1]) for e in ent}

    def run():
        tables = wf.cut(ent, brotli_amd.brotliDecode(comp))
        if state.get(b'glyf'):
            glyf, loca = brotli_amd.woff2_reconstruct_glyf(tables[b'glyf'])
            if state.get(b'hmtx'):
                ng = struct.unpack('>H', tables[b'glyf'][4:6])[0]
                nhm = struct.unpack('>H', tables[b'hhea'][34:36])[0]
                brotli_amd.woff2_reconstruct_hmtx(tables[b'hmtx'], glyf, loca, ng, nhm)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--file', default='enc-ttf-hmtx')
    ap.add_argument('--sequence', action='store_true')
    a = ap.parse_args()
    data = next(fx[1] for fx in wf.golden_files() if fx[0] == a.file)
    out = {'file': a.file, 'woff2_bytes': len(data), 'library': os.path.basename(os.path.dirname(brotli_amd.library_path()))}
    if a.sequence:
        out['sequence_ms_min_max'] = timed(sequence(data))
    else:
        out['sfnt_bytes'] = len(brotli_amd.woff2_decode(data))
        out['woff2_decode_ms_min_max'] = timed(lambda: brotli_amd.woff2_decode(data))
        brotli_amd.default_profiling(True)
        brotli_amd.woff2_decode(data)
        out['kernel_us'] = {k: round(v[0] * 1e3, 1) for k, v in sorted(brotli_amd.default_kernel_times().items())}
        brotli_amd.default_profiling(False)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
