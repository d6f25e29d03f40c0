"""The encoder's Huffman kernel alone (mib_debug_prefix_codes: huffman_kernel on fabricated
metablocks, through the encoder's own launch arithmetic) against the reference's
buildAndStoreHuffmanTree (the oracle's build_store_tree): for every histogram the serialised bits,
their count, the depths and the codes are equal.

The kernel restates createHuffmanTree (rank sort by the wave, two-queue merge by lane 0, count
limit doubling), convertBitDepthsToSymbols and the simple / complex serialisations; natural inputs
almost never reach their edge paths, so the histograms are chosen (tests/_prefix_code_cases.py;
tests/test_entropy_audit_host.py proves on the reference alone what they reach): no / one / two /
three / four (both shapes) / five used symbols, Fibonacci and power-of-two counts that need 1, 2,
4 and 5 count limits, all symbols equal (one code-length symbol), zero runs and equal-depth runs
around the run-length codes' corner cases (7, 11, past 138), one count of 2^24, and 300 seeded
random histograms per alphabet.  A launch's fabricated metablocks are full -- the literal slots
spread over eight block types, eight command types, eight distance types of four codes -- so the
second items of the kernel's blocks (command and distance types 4..7) run too.
"""
import functools

import pytest

import _oracle
import _prefix_code_cases as C
import brotli_amd

pytestmark = pytest.mark.gpu


def _check(cases):
    """one launch for all the cases; the mismatches"""
    got = brotli_amd.debug_prefix_codes([h for _, h in cases])
    assert len(got) == len(cases)
    bad = []
    for (name, h), g in zip(cases, got):
        want_bytes, want_bits, want_depths, want_codes = _oracle.build_store_tree(h)
        nb = (want_bits + 7) // 8
        why = []
        if g['bits'] != want_bits:
            why.append('bits %d, reference %d' % (g['bits'], want_bits))
        if g['bytes'][:nb] != want_bytes or any(g['bytes'][nb:]):
            why.append('serialised bytes differ')
        if g['depths'] != want_depths:
            why.append('depths differ at symbol %d' % next(i for i in range(len(h)) if g['depths'][i] != want_depths[i]))
        if g['codes'] != want_codes:
            why.append('codes differ at symbol %d' % next(i for i in range(len(h)) if g['codes'][i] != want_codes[i]))
        if why:
            bad.append((len(h), name, why))
    return bad


@functools.lru_cache(maxsize=1)
def _crafted():
    return [(name, h) for a in C.ALPHABETS for name, h in C.crafted(a)]


def test_chosen_histograms_equal_the_reference():
    cases = _crafted()
    for a in C.ALPHABETS:
        for name, h in cases:
            if len(h) == a and ('fibonacci' in name or 'powers' in name):
                print('%d %s: %d count limits' % (a, name, _oracle.create_huffman_tree(h)[1]))
    per = {a: sum(1 for _, h in cases if len(h) == a) for a in C.ALPHABETS}
    assert per[704] >= 8 and per[64] >= 32, per   # both items of the command and distance blocks
    bad = _check(cases)
    assert not bad, bad[:10]


def test_random_histograms_equal_the_reference():
    cases = [c for a in C.ALPHABETS for c in C.random_histograms(a, 300, 1000 + a)]
    retried = sum(1 for _, h in cases if _oracle.create_huffman_tree(h)[1] > 1)
    print('%d random histograms, %d needed more than one count limit' % (len(cases), retried))
    bad = _check(cases)
    assert not bad, (len(bad), bad[:10])


def test_rejects_other_alphabets():
    with pytest.raises(brotli_amd.BrotliError):
        brotli_amd.debug_prefix_codes([[1] * 100])
