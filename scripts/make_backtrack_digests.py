"""Record tests/golden/backtrack_digests.json: per case of tests/_backtrack_cases.py, each
stream's compressed size and SHA-256 as the loaded library (BROTLI_AMD_LIB) encodes it.  Run on
the GPU with the build of the commit BEFORE the backtrack's window walk moved to the vector side
(the build whose bytes that one and later builds must reproduce), never with a later one; the
commit it was recorded from goes in with --commit.
usage: BROTLI_AMD_LIB=<that commit's libbrotli_amd.so> \
           python3 scripts/make_backtrack_digests.py --commit HASH [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _backtrack_cases as cases  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--commit', required=True)
ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'backtrack_digests.json'))
args = ap.parse_args()
if not os.environ.get('BROTLI_AMD_LIB'):
    sys.exit('BROTLI_AMD_LIB must name the library of the commit given with --commit')
out = {'commit': args.commit, 'cases': {}}
for name in cases.CASES:
    out['cases'][name] = cases.digest(cases.encode(name))
    print(name, len(out['cases'][name]), 'streams', sum(d[0] for d in out['cases'][name]), 'bytes', file=sys.stderr, flush=True)
with open(args.out, 'w') as f:
    json.dump(out, f, indent=0)
    f.write('\n')
