"""The entropy audit (tests/_entropy_audit.py) on the HIP encoder's own streams: every prefix code
and both context maps of every compressed metablock are, bit for bit, what the reference's
buildAndStoreHuffmanTree / encodeContextMap write for the same histogram / map -- the codes'
lengths are createHuffmanTree's, no never-emitted symbol has a code, the run-length and
code-length coding and the context maps' run-length choice are the reference's.

Each case also asserts what it is there to reach, read from the oracle's trace, and that no
metablock was stored uncompressed (a stored metablock has nothing to audit: the cap keeps a case
from passing by skipping)."""
import functools

import numpy as np
import pytest

import _entropy_audit
import _oracle
import _split_inputs
import brotli_amd
from brotli_amd import datagen

pytestmark = pytest.mark.gpu


def _audit(enc, data, dictionary=None, what=''):
    findings, tr = _entropy_audit.audit_with_trace(enc, dictionary)
    assert tr['result'] == data, what
    assert findings == [], (what, findings[:6])
    assert tr['metablocks'][0] >= 1 and tr['metablocks'][1] == 0, (what, tr['metablocks'])
    return tr


def _used(code):
    return _entropy_audit.used_symbols(code)


@functools.lru_cache(maxsize=1)
def _text():
    return datagen.enwik_text(96 * 1024, 7)


@pytest.mark.parametrize('opts', [{'quality': 2}, {'quality': 5}, {'quality': 9}, {'quality': 10}, {'quality': 11},
                                  {'quality': 11, 'lgwin': 16}], ids=lambda o: 'q%d-lgwin%d' % (o['quality'], o.get('lgwin', 22)))
def test_text(opts):
    data = _text()
    tr = _audit(brotli_amd.brotliEncode(data, opts), data, what=opts)
    print('%s: %d codes, %d maps' % (opts, len(tr['codes']), len(tr['maps'])))


def test_glyph_data_font_mode():
    data = datagen.glyf_stream(128 * 1024, 1001)
    _audit(brotli_amd.brotliEncode(data, {'mode': brotli_amd.EncoderMode.FONT}), data)


def test_literal_codes_longer_than_8_bits():
    data = _split_inputs.lit_stress(65536, 500)
    tr = _audit(brotli_amd.brotliEncode(data), data)
    longest = max(max(_oracle.build_store_tree(c['hist'])[2]) for c in tr['codes'] if c['kind'] == _oracle.LITERAL)
    print('longest literal code length %d' % longest)
    assert longest > 8


def test_more_than_four_literal_types_and_eight_trees():
    data = _split_inputs.eight_alphabets()
    tr = _audit(brotli_amd.brotliEncode(data), data)
    types = max(c['alphabet'] - 2 for c in tr['codes'] if c['kind'] == _oracle.BLOCK_TYPE)
    ntrees = max(m['ntrees'] for m in tr['maps'])
    print('literal block types %d, most trees of a context map %d' % (types, ntrees))
    assert types > 4 and ntrees > 8


def test_more_than_four_command_or_distance_types():
    data = _split_inputs.kinds_input()
    tr = _audit(brotli_amd.brotliEncode(data), data)
    types = max(c['alphabet'] - 2 for c in tr['codes'] if c['kind'] in (_oracle.BLOCK_TYPE + 1, _oracle.BLOCK_TYPE + 2))
    print('most command / distance block types %d' % types)
    assert types > 4


def _small_batch():
    """70 compressible buffers of 64..5,000 bytes: periods of two, runs of one byte, short
    alphabets, text (long enough to compress), a phrase repeated"""
    nxt = datagen.xorshift32(4242)
    text = datagen.enwik_text(40000, 91)
    out = []
    for k in (32, 33, 100, 517, 1000, 2500):
        out.append(b'ab' * k)
    for n in (64, 65, 127, 1000, 4999):
        out.append(bytes([65 + n % 7]) * n)
    for n in (64, 80, 128, 200, 333, 512, 777, 1024, 1500, 2048, 3000, 4096, 5000):
        out.append(bytes(b'ACGT'[nxt() % 4] for _ in range(n)))
        out.append(bytes(b'01'[nxt() % 2] for _ in range(n)))
    for i, n in enumerate((600, 700, 800, 900, 1000, 1200, 1400, 1600, 1800, 2000, 2200, 2400, 2600, 2800, 3000, 3300,
                           3600, 3900, 4200, 4500, 4800, 5000)):
        out.append(text[1500 * i:1500 * i + n])
    for n in (64, 96, 150, 250, 400, 650, 1100, 1900, 3100, 4700, 5000):
        out.append((text[n:n + 24] * (n // 24 + 1))[:n])
    assert len(out) == 70 and all(64 <= len(b) <= 5000 for b in out)
    return out


def test_small_streams_reach_the_simple_forms():
    bufs = _small_batch()
    outs = brotli_amd.encode_batch(bufs)
    one = few = 0
    for i, (b, e) in enumerate(zip(bufs, outs)):
        tr = _audit(e, b, what=(i, len(b)))   # (every buffer has 64 bytes or more: none may be stored)
        one += sum(1 for c in tr['codes'] if _used(c) == 1)
        few += sum(1 for c in tr['codes'] if 2 <= _used(c) <= 4)
    print('codes with one used symbol %d, with two to four %d' % (one, few))
    assert one > 0 and few > 0


def test_streaming_encoder_metablocks():
    data = datagen.enwik_text(900000, 17)
    e = brotli_amd.BrotliEncoder({'quality': 9, 'lgwin': 18})
    parts = [e.update(data[p:p + 300000]) for p in range(0, len(data), 300000)]
    parts.append(e.finish())
    tr = _audit(b''.join(parts), data)
    print('metablocks (compressed, stored, metadata, empty) %s' % (tr['metablocks'],))
    assert tr['metablocks'][0] >= 3


def test_custom_dictionary():
    d = datagen.c5_dictionary()
    # the dictionary's tail at the stream start, where the window has nothing to offer, and again later
    data = (d[-180:] + datagen.enwik_text(40000, 3) + d[-97:] + datagen.enwik_text(65536, 4))[:65536]
    enc = brotli_amd.brotliEncode(data, {'customDictionary': d})
    before = _oracle.compound_refs()
    _audit(enc, data, dictionary=d)
    assert _oracle.compound_refs() > before   # (the stream does use the dictionary)


def test_power_of_two_symbol_frequencies():
    """256 KiB whose byte values have frequencies 1, 2, 4, ... 2^17, in seeded order: the literal
    histograms are what createHuffmanTree's count limit is for.  How many traced histograms needed
    a second count limit is printed, not asserted: the split and the clustering decide what the
    histograms are, and tests/test_gpu_prefix_codes.py covers that path for certain."""
    sym = np.repeat(np.arange(18, dtype=np.uint8) + 65, [1 << i for i in range(18)])
    data = (np.random.default_rng(18).permutation(sym).tobytes() + b'A')[:1 << 18]
    tr = _audit(brotli_amd.brotliEncode(data), data)
    retried = sum(1 for c in tr['codes'] if _oracle.create_huffman_tree(c['hist'])[1] > 1)
    print('%d of %d traced histograms needed a second count limit' % (retried, len(tr['codes'])))
