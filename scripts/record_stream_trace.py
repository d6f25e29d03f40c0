"""Records what only the host loop of a streaming session determines: how each call's output is
cut (the bytes update() holds back until the next call), the device passes and the re-decoded
bytes.  tests/golden/stream_solo_trace.json is this script's output from the library of the
commit named in it; tests/test_gpu_stream_decode.py::test_solo_trace_is_the_parents replays it.

    BROTLI_AMD_LIB=<that commit's libbrotli_amd.so> \
        python scripts/record_stream_trace.py --commit <hash> --out tests/golden/stream_solo_trace.json

The corpus is tests/test_gpu_stream_decode_batch.py's _streams(), the streams of at most 256 KiB
compressed; each is driven alone through BrotliDecoder.update() / finish() twice: in 4,096-byte
chunks with default options ('b4096'), and with that module's seeded cuts of
test_seeded_random_cuts and outWindow 64 KiB ('rand').  A call that raises is recorded as its
error code in place of a length.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'brotli-lib_amd', 'python'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import brotli_amd   # noqa: E402
import test_gpu_stream_decode_batch as B   # noqa: E402

MAX_COMPRESSED = 256 << 10


def schedules(i, name, data):
    """[(schedule, update sizes, options)] of the corpus' i-th stream"""
    return [('b4096', B._cuts_fixed(len(data), 4096), None),
            ('rand', B._cuts_random(len(data), 31 * i + len(name)), {'outWindow': B.WIN})]


def trace(data, sizes, opts):
    """(lens, passes, redecoded) of one session driven alone"""
    d = brotli_amd.BrotliDecoder(opts)
    lens, pos = [], 0
    for n in list(sizes) + [None]:
        try:
            lens.append(len(d.finish() if n is None else d.update(data[pos:pos + n])))
        except brotli_amd.BrotliError as e:
            lens.append(e.code)
        pos += n or 0
    return lens, d.passes, d.redecoded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', help='the commit the library was built from (default: HEAD of this checkout)')
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
    cases = []
    for i, (name, data, _) in enumerate(B._streams()):
        if len(data) > MAX_COMPRESSED:
            continue
        for schedule, sizes, opts in schedules(i, name, data):
            lens, passes, redecoded = trace(data, sizes, opts)
            cases.append({'name': name, 'schedule': schedule, 'lens': lens, 'passes': passes, 'redecoded': redecoded})
    with open(a.out, 'w') as f:
        f.write('{\n "what": "solo BrotliDecoder.update()/finish() per call: scripts/record_stream_trace.py",\n')
        f.write(' "commit": %s,\n "cases": [\n' % json.dumps(commit))
        f.write(',\n'.join('  ' + json.dumps(c, separators=(',', ':')) for c in cases))
        f.write('\n ]\n}\n')
    print('%d cases from %s -> %s' % (len(cases), commit, a.out))


if __name__ == '__main__':
    main()
