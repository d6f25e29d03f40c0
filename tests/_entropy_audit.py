"""The entropy stage's audit: every prefix code and both context maps of a brotli stream against
what the reference's own serialisers write for the same element.

audit(stream) decodes the stream with the oracle's trace on (oracle/oracle_decode.c: where each
prefix code's serialisation lies in the stream, and the histogram of the symbols later decoded
with it; both context maps as decoded) and returns a list of findings, empty when

  * for every prefix code of every kind -- literal, command, distance, the block type and block
    count codes of the three categories, the two context maps' codes -- the stream's bits
    [begin, end) are exactly the bits the reference's buildAndStoreHuffmanTree writes for that
    histogram over that alphabet (oracle build_store_tree): the code lengths are
    createHuffmanTree's, no symbol that is never decoded has a code, and the simple form, the
    run-length codes 16 / 17 and the code-length code are the reference's;
  * each coded context map, NTREES through the IMTF bit, is exactly what the reference's
    encodeContextMap writes for the decoded map (oracle encode_context_map);
  * no context map holds a run of more than 64 zeros after the move-to-front transform
    (zero_run_limit).  This one is a property of the engine, not of the format: it numbers its
    trees per block type, so a run ends with its block type's 64 (or 4) entries at the latest and
    the reference's RLEMAX cap of 6 is never what differs; a longer run is reported, not
    excused.  The reference itself clusters across block types and does write longer runs (80 in
    one of the host test's inputs), so the audit of its own streams passes zero_run_limit=None;
    the bit comparison above holds for those maps all the same.

No element of the engine's streams departs from the reference's serialiser on purpose, so no
element has the "no more bits than the reference" allowance: every comparison here is for equal
bits.

A finding is a dict: 'what' ('prefix code' / 'context map' / 'zero run' / 'decode'), 'kind'
(tests/_oracle.py KIND_NAMES, or 'literal' / 'distance' for a map), 'mb', 'index', and for a
mismatch the two bit strings' lengths and the first differing bit.
"""
import _oracle


def _bits(data, begin, end):
    """stream bits [begin, end) as an int (LSB = bit `begin`)"""
    if end <= begin:
        return 0
    b0, b1 = begin >> 3, (end + 7) >> 3
    v = int.from_bytes(data[b0:b1], 'little') >> (begin & 7)
    return v & ((1 << (end - begin)) - 1)


def _first_diff(a, b):
    x = a ^ b
    return (x & -x).bit_length() - 1 if x else -1


def mtf_zero_runs(values):
    """the longest run of zeros in the move-to-front transform of a context map"""
    mtf = list(range(256))
    longest = run = 0
    for v in values:
        j = mtf.index(v)
        if j:
            mtf.insert(0, mtf.pop(j))
            run = 0
        else:
            run += 1
            longest = max(longest, run)
    return longest


def audit_trace(stream, tr, zero_run_limit=64):
    """the findings of a trace (see the module docstring)"""
    findings = []
    if not isinstance(tr['result'], bytes):
        findings.append({'what': 'decode', 'kind': 'stream', 'mb': -1, 'index': 0, 'error': tr['result']})
    for c in tr['codes']:
        want_bytes, want_n, _, _ = _oracle.build_store_tree(c['hist'])
        got_n = c['end'] - c['begin']
        got = _bits(stream, c['begin'], c['end'])
        want = int.from_bytes(want_bytes, 'little')
        if got_n != want_n or got != want:
            findings.append({'what': 'prefix code', 'kind': _oracle.KIND_NAMES[c['kind']], 'mb': c['mb'],
                             'index': c['index'], 'alphabet': c['alphabet'], 'used': sum(1 for x in c['hist'] if x),
                             'bits': got_n, 'reference_bits': want_n, 'first_diff': _first_diff(got, want)})
    for m in tr['maps']:
        kind = 'literal' if m['kind'] == 0 else 'distance'
        want_bytes, want_n = _oracle.encode_context_map(m['values'], m['ntrees'])
        got_n = m['end'] - m['begin']
        got = _bits(stream, m['begin'], m['end'])
        want = int.from_bytes(want_bytes, 'little')
        if got_n != want_n or got != want:
            findings.append({'what': 'context map', 'kind': kind, 'mb': m['mb'], 'index': 0, 'ntrees': m['ntrees'],
                             'bits': got_n, 'reference_bits': want_n, 'first_diff': _first_diff(got, want)})
        if m['ntrees'] > 1 and zero_run_limit is not None:
            run = mtf_zero_runs(m['values'])
            if run > zero_run_limit:
                findings.append({'what': 'zero run', 'kind': kind, 'mb': m['mb'], 'index': 0, 'run': run})
    return findings


def audit(stream, dictionary=None, zero_run_limit=64):
    """the findings of one stream; [] when every element is the reference's"""
    return audit_trace(stream, _oracle.trace(stream, dictionary), zero_run_limit)


def audit_with_trace(stream, dictionary=None, zero_run_limit=64):
    """(findings, trace): for tests that also read the trace (which paths the stream reached)"""
    tr = _oracle.trace(stream, dictionary)
    return audit_trace(stream, tr, zero_run_limit), tr


def used_symbols(code):
    return sum(1 for x in code['hist'] if x)
