"""HIP decoder parity (through the C ABI) against the reference's golden data and the oracle."""
import base64
import hashlib
import json
import os
import random

import pytest

import _inputs
import _oracle
import brotli_amd

pytestmark = pytest.mark.gpu
G = _inputs.GOLDEN


def _cases(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)['cases']


def test_canonical_vectors_bit_exact():
    n = 0
    for nm in sorted(os.listdir(os.path.join(G, 'vectors'))):
        if '.compressed' not in nm:
            continue
        with open(os.path.join(G, 'vectors', nm), 'rb') as f:
            comp = f.read()
        with open(os.path.join(G, 'vectors', nm.split('.compressed')[0]), 'rb') as f:
            exp = f.read()
        assert brotli_amd.brotliDecode(comp) == exp, nm
        n += 1
    assert n == 45


def test_bench_streams_match_reference_hashes():
    for c in _cases('decode_vectors.json'):
        with open(os.path.join(G, c['path']), 'rb') as f:
            out = brotli_amd.brotliDecode(f.read())
        assert hashlib.sha256(out).hexdigest() == c['sha256'], c['path']


def test_error_corpus_matches_reference():
    """same bytes or the same 'Brotli error code: N' as the reference on ~700 corrupted streams"""
    for c in _cases('decode_errors.json'):
        data = base64.b64decode(c['in_b64'])
        if c.get('hang'):
            # the reference never returns (Bug J); we return what the oracle (Bug J fixed) returns
            exp = _oracle.decode(data)
        elif 'error' in c:
            exp = c['error']
        else:
            exp = c['sha256']
        try:
            got = hashlib.sha256(brotli_amd.brotliDecode(data)).hexdigest()
        except brotli_amd.BrotliError as e:
            got = str(e)
        if isinstance(exp, int):
            exp = 'Brotli error code: %d' % exp
        elif isinstance(exp, bytes):
            exp = hashlib.sha256(exp).hexdigest()
        assert got == exp, (c['in_b64'][:60], got, exp)


def test_batch_decode_matches_oracle():
    streams, exps = [], []
    for nm in sorted(os.listdir(os.path.join(G, 'vectors'))):
        if '.compressed' in nm:
            with open(os.path.join(G, 'vectors', nm), 'rb') as f:
                streams.append(f.read())
            exps.append(_oracle.decode(streams[-1]))
    outs = brotli_amd.decode_batch(streams)
    assert outs == exps


def test_mixed_batch_with_and_without_a_dictionary_handle():
    """One list through decode_batch(...) and decode_batch(..., dictionary=d), d a small dictionary
    no stream refers to: an empty input, a one-metablock stream, a two-metablock stream of 1 MiB of
    zeros (25 bytes: its slot is 8x that, so it outgrows it and is decoded again alone), the same
    cut 10 bytes short, and a part-indexed stream.  Same bytes and the same error from both; the
    indexed stream decodes on one wave in the plain call's launch and part-parallel, alone, with
    the handle."""
    import _streams
    half = 1 << 19
    zeros = _streams.build(_streams.Stream(22, [_streams.MB('cmds', cmds=[(b'\0', half - 1, ('dist', 1))]) for _ in range(2)],
                                           'zeros_1mib')).data
    one = _streams.build(_streams.long_run(700, lgwin=16)).data
    with open(os.path.join(G, 'parts', 'parts_enwik300k.br'), 'rb') as f:
        indexed = f.read()
    streams = [b'', one, zeros, zeros[:-10], indexed]
    exps = [_oracle.decode(s) for s in streams]
    assert isinstance(exps[0], int) and exps[1] == b'r' * 700 and exps[2] == bytes(2 * half) and isinstance(exps[3], int)
    assert len(exps[4]) == 300000 and len(zeros) * 8 < 1 << 16

    def check(outs):
        got = [o.code if isinstance(o, brotli_amd.BrotliError) else o for o in outs]
        print([g if isinstance(g, int) else len(g) for g in got])
        assert got == exps

    before = brotli_amd.part_stats()
    check(brotli_amd.decode_batch(streams))
    assert brotli_amd.part_stats() == before
    with brotli_amd.Dictionary(bytes(range(256)) * 4) as d:
        check(brotli_amd.decode_batch(streams, dictionary=d))
    after = brotli_amd.part_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)


def test_decode_options_semantics():
    """maxOutputSize (decode.ts:46-62), legacy outputSize truncation / zero padding (engine.ts:2210-2220)"""
    with open(os.path.join(G, 'vectors', 'alice29.txt.compressed'), 'rb') as f:
        comp = f.read()
    with open(os.path.join(G, 'vectors', 'alice29.txt'), 'rb') as f:
        plain = f.read()
    with pytest.raises(brotli_amd.BrotliError, match='exceeds limit'):
        brotli_amd.brotliDecode(comp, {'maxOutputSize': 1000})
    assert brotli_amd.brotliDecode(comp, {'maxOutputSize': len(plain)}) == plain
    assert brotli_amd.brotliDecode(comp, 100) == _oracle.decode(comp, 100) == plain[:100]
    assert brotli_amd.brotliDecode(comp, len(plain) + 50) == _oracle.decode(comp, len(plain) + 50)


def test_random_truncations_match_oracle():
    rng = random.Random(7)
    with open(os.path.join(G, 'bench', 'enc-ttf.br'), 'rb') as f:
        comp = f.read()
    for _ in range(40):
        cut = rng.randrange(len(comp))
        data = comp[:cut]
        exp = _oracle.decode(data)
        try:
            got = brotli_amd.brotliDecode(data)
        except brotli_amd.BrotliError as e:
            got = e.code
        assert got == exp, cut


def test_compound_dictionary_matches_reference():
    """brotliDecode(data, {customDictionary}) against the reference's own outputs and errors
    (tests/golden/decode_compound.json), the dictionary given as bytes and as signed int8."""
    import array
    n = 0
    for c in _cases('decode_compound.json'):
        data = base64.b64decode(c['in_b64'])
        d = _inputs.resolve(c['dict'])
        dic = array.array('b', d) if c['int8'] else d
        try:
            got = hashlib.sha256(brotli_amd.brotliDecode(data, {'customDictionary': dic})).hexdigest()
        except brotli_amd.BrotliError as e:
            got = e.code if 'subarray' in c.get('error', '') else str(e)
        if 'error' not in c:
            assert got == c['sha256'], c
            n += 1
        elif c['error'].startswith('Brotli error code'):
            assert got == c['error'], (c, got)
        else:
            assert got == -106, (c, got)   # MIB_E_JS_TYPE_ERROR: the reference's TypeError
    assert n > 100
