"""A prepared dictionary's arithmetic without a GPU: brotli-lib_amd/csrc/shared_dict.h (what the
match finder's lookup and the decoder include) built as host code with AddressSanitizer and UBSan
into a stand-alone program (tests/shared_dict_host_main.cpp); and the Python statement of the
standard rule (tests/_shared_dict.py) against _streams' writer on a hand-checked stream."""
import os
import shutil
import subprocess

import pytest

import _shared_dict as sd
import _streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('shared_dict') / 'shared_dict_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'shared_dict_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith('ok ') and int(r.stdout.split()[1]) > 0
    return int(r.stdout.split()[1])


@pytest.mark.parametrize('seed', [1, 2])
def test_measure_and_cap_on_random_dictionaries(driver, seed):
    """every (position, address, length): equal bytes, inside the dictionary, inside the segment,
    at most kLongCopy, and maximal under those caps"""
    assert _run(driver, 'measure', str(seed)) > 100000


def test_distance_address_round_trip_around_max_backward(driver):
    _run(driver, 'roundtrip')


def test_edge_addresses_and_the_padding_trap(driver):
    _run(driver, 'edges')


def test_model_and_writer_agree_on_a_hand_checked_stream():
    """dictionary 100..196 (97 bytes), lgwin 16:
      'ab', copy 5 at distance 2 + 97 - 3 = 96    -> max distance 2, address 96 - 2 - 1 - 97 = -4,
                                                      offset 3: bytes 103..107
      '',   copy 4 with code 0 (distance 96 again) -> max distance 7, address -9, offset 8: 108..111;
                                                      pushed again: the ring is 96, 96, 4, 11
      'c',  copy 3 at distance 2                   -> the window: 111 'c' 111
      'd',  copy 2 with code 2 (ring[2] = 96)      -> max distance 16, address -18, offset 17: 117 118
      '.'"""
    D = bytes(range(100, 197))
    cmds = [(b'ab', 5, ('dist', 96)), (b'', 4, ('short', 0)), (b'c', 3, ('dist', 2)), (b'd', 2, ('short', 2)), (b'.', 2, None)]
    stream = sd.one(16, cmds)
    want = b'ab' + bytes(range(103, 112)) + b'c' + bytes([111]) + b'c' + bytes([111]) + b'd' + bytes([117, 118]) + b'.'
    assert sd.model(stream, D) == (want, None)
    built = sd.build(stream, D)
    assert built.sim_out == want
    assert sd.distance_of(2, 16, len(D), 3) == 96
    # without the dictionary's copies the description is _streams' own: the two models agree
    plain = sd.one(16, [(b'abcd', 3, ('dist', 2)), (b'.', 2, None)])
    assert sd.model(plain, D)[0] == _streams.model(plain) and sd.build(plain, D).data == _streams.build(plain).data
    # one byte past the dictionary's end
    bad = sd.one(16, [(b'ab', 6, ('dist', 2 + 5)), (b'.', 2, None)])   # offset 92, 6 bytes: 92 + 6 > 97
    assert sd.model(bad, D) == (b'ab', -9)
    # every case the GPU test decodes: the writer's own output is the model's
    for name, s, dic in sd.decoder_cases():
        out, err = sd.model(s, dic)
        b = sd.build(s, dic)
        assert (b.sim_out == out) if err is None else (b.sim_out[:len(out)] == out and name == 'one_past_the_end'), name
