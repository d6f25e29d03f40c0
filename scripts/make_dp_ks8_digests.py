"""Record tests/golden/dp_ks8_digests.json: per case of tests/_dp_ks8_cases.py, each stream's
compressed size and SHA-256 as the loaded library (BROTLI_AMD_LIB, or the tree's own) encodes
it.  Run on the GPU with the build whose bytes later builds must reproduce; the commit it was
recorded from goes in with --commit.
usage: python3 scripts/make_dp_ks8_digests.py --commit HASH [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _dp_ks8_cases as cases  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--commit', required=True)
ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'dp_ks8_digests.json'))
args = ap.parse_args()
out = {'commit': args.commit, 'cases': {}}
for name in cases.CASES:
    out['cases'][name] = cases.digest(cases.encode(name))
    print(name, len(out['cases'][name]), 'streams', sum(d[0] for d in out['cases'][name]), 'bytes', file=sys.stderr, flush=True)
with open(args.out, 'w') as f:
    json.dump(out, f, indent=0)
    f.write('\n')
