"""Inputs whose windows hold few copy nodes, for choosing kBtVecMin (enc_parse.hip: windows
with fewer copy nodes than that are walked on the scalar side).  512 streams of 1 MiB of random
bytes into which copies of 6 bytes (from 1,000 bytes back) are written at DENSITY copies per 64
positions, for a list of densities; each batch is encoded twice.  Run under
`rocprofv3 --kernel-trace` with the experiments build (BROTLI_AMD_LIB), once per
MIB_BT_VEC_MIN: the trace's backtrack_kernel launches are, in order, four per call (two encode
lanes, each the sampled first pass and then the pieces) and eight per density.
usage: MIB_BT_VEC_MIN=N BROTLI_AMD_LIB=<experiments build> \
           rocprofv3 --kernel-trace -d DIR -o run -f csv -- python3 scripts/backtrack_threshold.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import brotli_amd  # noqa: E402

MIB = 1 << 20
K = 512
DENSITIES = (0.0, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0)


def stream(density, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, MIB, dtype=np.uint8)
    if density:
        step = 64.0 / density
        at = (np.arange(int((MIB - 2000) / step)) * step).astype(np.int64) + 1500
        at += rng.integers(0, max(int(step) - 6, 1), len(at))
        for q in range(6):   # (ascending positions: a source already written stays a copy)
            d[at + q] = d[at + q - 1000]
    return d


dev = torch.device('cuda', 0)
ctx = brotli_amd.DeviceContext(0)
cap = K * MIB + K * MIB // 8 + 4096 * K
comp = torch.empty(cap, dtype=torch.uint8, device=dev)
offs = [i * MIB for i in range(K + 1)]
sizes = {}
for density in DENSITIES:
    data = torch.from_numpy(stream(density, 77)).to(dev).repeat(K)
    torch.cuda.synchronize()
    for it in range(2):
        off = ctx.encode(data.data_ptr(), offs, comp.data_ptr(), cap, {'quality': 11})
    sizes[str(density)] = off[1] - off[0]
print(json.dumps({'vec_min': os.environ.get('MIB_BT_VEC_MIN'), 'streams': K, 'densities': DENSITIES, 'stream_bytes': sizes}))
