"""The host planning of a one-shot decode without a GPU: brotli-lib_amd/csrc/decode_plan.h (window
bits, the announced size, the part index reader and a host batch's layout, as runtime.cpp uses
them) built as host code with AddressSanitizer and UBSan into a stand-alone program
(tests/decode_plan_host_main.cpp) and run as a child process.  The streams it reads are untrusted
and live in heap blocks of their exact lengths: a byte read past one ends the program."""
import os
import shutil
import subprocess

import pytest

import _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'parts', 'parts_enwik300k.br')


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = str(tmp_path_factory.mktemp('decode_plan') / 'decode_plan_host')
    subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-Wall', '-Werror', '-I', os.path.join(ROOT, 'brotli-lib_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'decode_plan_host_main.cpp'), '-o', exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[-1].startswith('ok ') and int(lines[-1].split()[1]) > 0
    return lines[:-1], int(lines[-1].split()[1])


def test_fixture_plan_equals_the_python_reader(driver):
    """every entry of parts_enwik300k.br's chain, its total and window bits, as _parts.read_chain
    reads them; and the stream looks indexed"""
    with open(FIXTURE, 'rb') as f:
        stream = f.read()
    ents, total = _parts.read_chain(stream)
    head, _ = _parts.read_index(stream)
    lines, _ = _run(driver, 'golden', FIXTURE)
    assert lines[0].split() == ['plan', str(len(ents)), str(total), str(int(head['lgwin'])), '1']
    assert (len(ents), total, int(head['lgwin'])) == (5, 300000, 22)
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[1:]]
    want = [(int(e['bit']), int(e['pos']), int(e['mb_bit']), int(e['mb_pos']), int(e['flags'])) for e in ents]
    assert got == want


def test_hand_built_chains_accepted_and_one_rejected_per_rule(driver):
    """lgwin 16, 17 and 22 (window bits of 1, 7 and 4 bits): one block, two blocks through next_byte
    and a lone final 0x03 are accepted with the entries they were built from; a chain breaking one
    rule of read_part_index / plan_parts is rejected, for every rule"""
    _, checks = _run(driver, 'chains')
    assert checks > 3 * 30


def test_bit_flips_and_truncations_never_read_past_the_stream(driver):
    """every single-bit flip in the first 2,048 bytes and every truncation to 0..3,000 bytes, of the
    fixture and of a hand-built chain, through plan_parts and looks_indexed: no sanitizer report,
    and an accepted plan keeps the entry rules.  (Acceptance itself is the device's to settle:
    most flips land in fields only the kernel checks.)"""
    lines, checks = _run(driver, 'robust', FIXTURE)
    print(lines[-1])
    assert checks >= 8 * 2048 + 3001


def test_window_bits_and_announced_size_on_every_two_byte_prefix(driver):
    """all 65,536 prefixes: the one window-bits decoder (on both bit readers) against RFC 7932
    section 9.1's table; peek_window_bits is the window's log2, 24 for the large-window escape;
    decoded_size, alone and in front of fixed tails, is section 9.2's header read by the test"""
    _, checks = _run(driver, 'window')
    assert checks >= 65536 * 8


def test_batch_layout_classes_offsets_and_totals(driver):
    """empty input, a header-sized stream, streams without an announced size, one announcing more
    than maxOutputSize, the largest announcement there is, and the indexed fixture; with and without
    the alone rules and the limit: how each is handled, 256-aligned slots that do not overlap and
    hold capacity + MIB_IN_PLACE_SLACK + 64, and the two totals"""
    _run(driver, 'layout', FIXTURE)
