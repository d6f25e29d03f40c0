"""The match search's passes after the candidate walk -- static-dictionary words, the custom
dictionary's tail copies, the near scan (dict_matches_kernel, cdict_matches_kernel,
near_matches_kernel, enc_match.hip) -- record word for record word against the plain references
of tests/_match_passes.py, through mib_debug_match_passes, which runs them as an encode call
does.  What each case is there for is asserted on the references alone in
tests/test_match_passes_host.py."""
import numpy as np
import pytest

import brotli_amd
import _match_passes as mp
from test_match_passes_host import reached


def differing(got, want):
    return np.flatnonzero((got != want).any(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize('name', mp.CASES)
def test_match_passes(name):
    bufs, opt, passes, history = mp.case(name)
    got = brotli_amd.debug_match_records(bufs, opt, passes=passes, history=history)
    want, _ = mp.expected(name)
    assert reached(name)   # the case holds what it is there for (the reference's records alone)
    assert len(got) == len(want)
    for s, (gt, wt) in enumerate(zip(got, want)):
        assert gt.shape == wt.shape, (name, s)
        bad = differing(gt, wt)
        assert bad.size == 0, '%s stream %d (%d bytes): %d records differ, first at %d: got %s want %s' % (
            name, s, len(wt), bad.size, bad[0], [hex(x) for x in gt[bad[0]]], [hex(x) for x in wt[bad[0]]])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['gate_q9', 'gate_font', 'words_lgwin24', 'words_q9', 'words_history'])
def test_gated_pass_changes_nothing(name):
    """the library's own records with the pass asked for and without it"""
    bufs, opt, passes, history = mp.case(name)
    with_pass = brotli_amd.debug_match_records(bufs, opt, passes=passes, history=history)
    without = brotli_amd.debug_match_records(bufs, opt, passes=0, history=history)
    for a, b in zip(with_pass, without):
        assert (a == b).all(), name


@pytest.mark.gpu
def test_no_pass_is_the_walk():
    """passes = 0 and history = 0 through the new entry: mib_debug_match_records' records"""
    bufs, opt, _, _ = mp.case('mixed_q11_lgwin22')
    _, stages = mp.expected('mixed_q11_lgwin22')
    for gt, st in zip(brotli_amd.debug_match_records(bufs, opt), stages):
        assert differing(gt, st['walk']).size == 0
