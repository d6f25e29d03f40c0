"""The entropy audit and the oracle's trace, without a GPU.

  * The audit (tests/_entropy_audit.py) is empty on the oracle's own encodes: the reference
    satisfies its own serialisers by construction, so an empty audit proves the trace's bit
    ranges and histograms, for every kind of code and both context maps.
  * Two written streams (tests/_streams.py) that decode but are not the reference's: each gives
    exactly its finding.
  * The crafted histograms of tests/_prefix_code_cases.py reach what they are for, read from the
    reference alone: how many count limits createHuffmanTree tries, the depths, the runs.
  * The trace on malformed streams, in a stand-alone program under AddressSanitizer and UBSan
    (tests/oracle_trace_host_main.c with the oracle's sources; nothing loaded into Python).
"""
import base64
import functools
import json
import os
import shutil
import struct
import subprocess

import pytest

import _entropy_audit
import _oracle
import _prefix_code_cases as C
import _split_inputs
import _streams as S
from brotli_amd import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, FONT = 0, 2


@functools.lru_cache(maxsize=None)
def _input(name):
    if name == 'text':
        return datagen.enwik_text(96 * 1024, 7)
    if name == 'glyf':
        return datagen.glyf_stream(128 * 1024, 1001)
    if name == 'eight alphabets':
        return _split_inputs.eight_alphabets()
    return _split_inputs.kinds_input()


@pytest.mark.parametrize('mode', [GENERIC, FONT])
@pytest.mark.parametrize('name', ['text', 'glyf', 'eight alphabets', 'kinds'])
def test_audit_is_empty_on_the_oracles_own_encodes(name, mode):
    data = _input(name)
    for q in (5, 9, 10, 11):
        enc = _oracle.encode(data, q, 22, mode)
        # (zero_run_limit: the bound on zero runs is the engine's property; the reference clusters
        # across block types and has longer ones -- _entropy_audit's docstring)
        findings, tr = _entropy_audit.audit_with_trace(enc, zero_run_limit=None)
        assert tr['result'] == data, (name, mode, q)
        assert findings == [], (name, mode, q, findings[:4])
        assert tr['metablocks'][0] >= 1 and len(tr['maps']) == 2 * tr['metablocks'][0]
        kinds = sorted({c['kind'] for c in tr['codes']})
        print('%s mode %d q%d: %d bytes, %d codes of kinds %s, metablocks %s' % (name, mode, q, len(enc), len(tr['codes']),
                                                                                 kinds, tr['metablocks']))


def test_the_oracles_encodes_cover_every_kind_of_code():
    """over the inputs above some encode has every kind of record: the three symbol alphabets, the
    block type and block count codes of the three categories, both context maps' codes"""
    kinds = set()
    for name in ('text', 'eight alphabets', 'kinds'):
        tr = _oracle.trace(_oracle.encode(_input(name), 9, 22, GENERIC))
        kinds |= {c['kind'] for c in tr['codes']}
    assert kinds == set(range(11)), sorted(kinds)


# ---------------------------------------------------------------- negative controls
def _skewed_literals_stream():
    """one metablock: one command code (one symbol), one distance code (one symbol), and one literal
    code over eight symbols of very unequal counts, written flat (_streams.balanced)"""
    law = b'a' * 40 + b'b' * 20 + b'c' * 10 + b'd' * 5 + b'e' * 2 + b'fgh'
    lits = bytes(law[(k * 37) % len(law)] for k in range(400))
    cmds = [(lits[5 * k:5 * k + 5], 2, ('short', 0)) for k in range(79)] + [(lits[395:400], 2, None)]
    return S.Stream(16, [S.MB('cmds', cmds=cmds)], 'skewed_literals')


def _plain_map_stream():
    """one metablock whose literal context map (two trees: contexts 0..31 and 32..63) is written
    with RLEMAX 0, a symbol per entry, although its move-to-front form is two runs of zeros; every
    prefix code has one symbol (two for the map's own code, in the reference's order)"""
    mb = S.MB('cmds', cmds=[(b'\x21\x01\x21\x01', 2, ('short', 0))] * 30 + [(b'\x21\x01\x21\x01', 2, None)])
    mb.modes = [S.LSB6]
    mb.ntrees_l, mb.lmap = 2, [0] * 32 + [1] * 32
    mb.lmap_rle, mb.lmap_imtf = 0, True
    mb.shapes = {('LM', 0): {'sorted': True}}
    return S.Stream(16, [mb], 'plain_map')


def test_a_flat_code_over_a_skewed_histogram_is_the_one_finding():
    st = _skewed_literals_stream()
    built = S.build(st)
    findings, tr = _entropy_audit.audit_with_trace(built.data)
    assert tr['result'] == S.model(st)
    lit = [c for c in tr['codes'] if c['kind'] == _oracle.LITERAL]
    assert len(lit) == 1 and _entropy_audit.used_symbols(lit[0]) == 8
    assert [(f['what'], f['kind'], f['index']) for f in findings] == [('prefix code', 'literal', 0)], findings
    assert findings[0]['bits'] != 0 and findings[0]['first_diff'] >= 0


def test_a_context_map_without_run_lengths_is_the_one_finding():
    st = _plain_map_stream()
    built = S.build(st)
    assert built.stats['map_plain'] == 1 and built.stats['map_imtf'] == 1
    findings, tr = _entropy_audit.audit_with_trace(built.data)
    assert tr['result'] == S.model(st)
    lmap = [m for m in tr['maps'] if m['kind'] == 0][0]
    assert lmap['ntrees'] == 2 and lmap['values'] == [0] * 32 + [1] * 32
    assert _entropy_audit.mtf_zero_runs(lmap['values']) == 32
    assert [(f['what'], f['kind']) for f in findings] == [('context map', 'literal')], findings
    assert findings[0]['bits'] > findings[0]['reference_bits']


def test_a_zero_run_past_64_is_reported():
    """(the engine's maps never have one; the audit says so when it meets one, even where the
    map's bits are the reference's)"""
    assert _entropy_audit.mtf_zero_runs([0] * 64 + [1] + [1] * 64) == 64
    assert _entropy_audit.mtf_zero_runs([0] * 65 + [1]) == 65
    values = [0] * 100 + [1] * 28
    data, nbits = _oracle.encode_context_map(values, 2)
    tr = {'result': b'', 'codes': [], 'maps': [{'kind': 0, 'mb': 0, 'size': 128, 'ntrees': 2, 'begin': 0, 'end': nbits,
                                                 'values': values}]}
    findings = _entropy_audit.audit_trace(data, tr)
    assert [(f['what'], f['kind'], f['run']) for f in findings] == [('zero run', 'literal', 100)], findings
    assert _entropy_audit.audit_trace(data, tr, zero_run_limit=None) == []


# ---------------------------------------------------------------- reach of the crafted histograms
def _attempts(counts, limit=15):
    return _oracle.create_huffman_tree(counts, limit)


def test_count_limit_retries_of_the_crafted_histograms():
    d, n = _attempts(C.fibonacci(16))
    assert n == 1 and max(d) == 15
    assert _attempts(C.fibonacci(17))[1] == 2
    assert sum(C.fibonacci(32)) == 5702886 and _attempts(C.fibonacci(32))[1] == 5
    assert _attempts(C.powers_of_two(18))[1] == 4
    # scattered or packed, in every alphabet: the same retries (the order of the symbols decides ties only)
    for a in C.ALPHABETS:
        got = {name: _attempts(h)[1] for name, h in C.crafted(a) if 'fibonacci' in name or 'powers' in name}
        for name, n in got.items():
            want = {'fibonacci 16': 1, 'fibonacci 17': 2, 'fibonacci 32': 5, 'powers of two 18': 4}[name.split(',')[0]]
            assert n == want, (a, name, n)
    # the code-length code's limit of 5
    assert _attempts(C.fibonacci(8) + [0] * 10, 5)[1] == 2


def test_equal_counts_give_one_code_length_symbol():
    """256 equal counts: every depth 8, so the run-length codes are repeats of the initial
    'previous length' 8 alone -- four codes 16 -- and the code-length histogram has one used
    symbol: HSKIP 3, fifteen code-length lengths (fourteen zeros of 2 bits, one 4-bit '1'), then
    four times zero bits and two extra bits: 42 bits"""
    data, nbits, depths, codes = _oracle.build_store_tree([5] * 256)
    assert depths == [8] * 256 and sorted(codes) == list(range(256))
    assert nbits == 2 + (14 * 2 + 4) + 4 * 2 and data[0] & 3 == 3
    # 704 equal counts: 320 codes of 9 bits and 384 of 10
    _, _, depths, _ = _oracle.build_store_tree([1] * 704)
    assert sorted(set(depths)) == [9, 10] and depths.count(9) == 320


def test_crafted_runs_are_in_the_references_depths():
    """the zero runs and the equal-depth runs the cases are named for, read from the reference's
    depths (runs between used symbols: the trailing zeros are not coded)"""
    for a in C.ALPHABETS:
        zero, equal = set(), set()
        for name, h in C.crafted(a):
            _, _, depths, _ = _oracle.build_store_tree(h)
            while depths and depths[-1] == 0:
                depths.pop()
            for v, n in C.runs_of(depths):
                if name.startswith('zero runs') and v == 0:
                    zero.add(n)
                if name == 'equal-depth run of %d' % n and v:
                    equal.add(n)
        assert zero >= {r for r in C.ZERO_RUNS if r + 6 <= a}, (a, sorted(zero))
        assert equal == {r for r in C.DEPTH_RUNS if C.depth_run(r, a) is not None}, (a, sorted(equal))
        assert equal >= {1, 2, 3, 4, 5, 6, 7, 8, 11}
    assert C.depth_run(70, 256) is not None and C.depth_run(70, 704) is not None


def test_crafted_cases_fill_both_items_of_the_kernels_blocks():
    """eight command types and eight distance types of four codes per fabricated metablock: more
    cases than that in each alphabet, so the slots of types 4..7 are filled too"""
    assert len(C.crafted(704)) >= 8 and len(C.crafted(64)) >= 32 and len(C.crafted(256)) >= 24


# ---------------------------------------------------------------- the trace on malformed input
def test_trace_on_malformed_streams_under_sanitizers(tmp_path):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc is not None, 'the oracle is built with a C compiler: there is none'
    with open(os.path.join(ROOT, 'tests', 'golden', 'decode_errors.json')) as f:
        streams = [base64.b64decode(c['in_b64']) for c in json.load(f)['cases']]
    whole = S.build(S.many_types()).data
    cuts = sorted({1 + (len(whole) - 2) * k // 39 for k in range(40)})
    assert len(cuts) == 40
    streams += [whole[:n] for n in cuts] + [whole]
    pack = tmp_path / 'streams.bin'
    with open(pack, 'wb') as f:
        for s in streams:
            f.write(struct.pack('<I', len(s)) + s)
    exe = str(tmp_path / 'oracle_trace_host')
    odir = os.path.join(ROOT, 'oracle')
    subprocess.run([cc, '-std=gnu11', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-ffp-contract=off', '-I', odir, os.path.join(ROOT, 'tests', 'oracle_trace_host_main.c'),
                    os.path.join(odir, 'oracle_decode.c'), os.path.join(odir, 'oracle_encode.c'), '-lm', '-o', exe],
                   check=True)
    r = subprocess.run([exe, str(pack)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    got = dict(zip(words[0::2], (int(x) for x in words[1::2])))
    assert got['streams'] == len(streams) and got['bad'] == 0, r.stdout
    assert got['failed'] >= 40 and got['codes'] > 0 and got['maps'] > 0, r.stdout
