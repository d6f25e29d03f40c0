"""A prepared dictionary's addressing ("standard": brotli_amd.h, mib_dictionary), stated in plain
Python, and the means to write streams that use it.

The decoder's arithmetic is the custom dictionary's: a copy whose distance exceeds the maximum
distance max_d = min(bytes decoded so far, 2^lgwin - 16) has the address

    address = distance - max_d - 1 - len(dictionary)

and a negative address is a copy from dictionary offset a = -address - 1.  With a prepared
dictionary that copy is valid when a + length <= len(dictionary), and the stream fails with -9
otherwise.  Valid or not it pushes its distance on the ring of last distances, whatever code the
distance came with (code 0 included).  An address >= 0 names a static-dictionary word, which the
model leaves out (no stream here uses one beside a dictionary).

model() decodes a description of tests/_streams.py (Stream / MB) by these rules alone.  build()
serialises one with _streams' own writer; only the writer's idea of a copy (State.copy, which
knows no distance beyond the window) is replaced, by DictState."""
import random

import _streams as S

ERR_COPY = -9


def max_backward(lgwin):
    return (1 << lgwin) - 16


def distance_of(pos, lgwin, dict_len, a):
    """the distance that addresses dictionary offset a from stream position pos"""
    return min(pos, max_backward(lgwin)) + (dict_len - a)


def model(stream, dictionary):
    """(decoded bytes, None), or (the bytes decoded before the failing copy, -9)"""
    out, ring = bytearray(), [4, 11, 15, 16]
    for mb in stream.mbs:
        if mb.kind == 'raw':
            out += mb.data
        for ins, n, spec in (mb.cmds if mb.kind == 'cmds' else []):
            out += ins
            if spec is None:
                continue
            assert spec[0] != 'word'
            if spec[0] == 'implicit':
                d = ring[0]
            elif spec[0] == 'short':
                d = ring[S.SHORT_IDX[spec[1]]] + S.SHORT_DELTA[spec[1]]
            else:
                d = spec[1]
            max_d = min(len(out), max_backward(stream.lgwin))
            if d > max_d:
                address = d - max_d - 1 - len(dictionary)
                assert address < 0, 'a static-dictionary word'
                a = -address - 1
                if a + n > len(dictionary):
                    return bytes(out), ERR_COPY
                out += dictionary[a:a + n]
                ring = [d] + ring[:3]
                continue
            if spec not in (('implicit',), ('short', 0)):
                ring = [d] + ring[:3]
            for _ in range(n):
                out.append(out[len(out) - d])
    return bytes(out), None


class DictState(S.State):
    """_streams.State with the dictionary in front of the stream"""

    def __init__(self, lgwin, dictionary):
        super().__init__(lgwin)
        self.dictionary = bytes(dictionary)
        self.failed = False

    def copy(self, spec, copy_len):
        d, code, _, n = self.resolve(spec, copy_len)
        if spec[0] == 'word' or d <= self.maxd():
            return super().copy(spec, copy_len)
        a = -(d - self.maxd() - 1 - len(self.dictionary)) - 1
        assert a >= 0, 'a static-dictionary word'
        if a + n > len(self.dictionary):
            self.failed = True   # (the stream is still written whole: bytes that no decoder reaches)
        self.out += (self.dictionary[a:a + n] + bytes(n))[:n]
        self.ring = [d] + self.ring[:3]
        return d, code


def build(stream, dictionary):
    """the stream's bytes (metablocks of kind 'cmds' and 'empty'), written by _streams' writer"""
    bw, st, s = S.BitWriter(), S.new_stats(), DictState(stream.lgwin, dictionary)
    rng = random.Random(stream.seed * 7919 + 1)
    w = stream.lgwin
    if w == 16:
        bw.put(0, 1)
    elif w >= 18:
        bw.put(1 | ((w - 17) << 1), 4)
    elif w == 17:
        bw.put(1, 7)
    else:
        bw.put(1 | ((w - 8) << 4), 7)
    for k, mb in enumerate(stream.mbs):
        last = k == len(stream.mbs) - 1
        if mb.kind == 'empty':
            assert last
            bw.put(3, 2)
        else:
            assert mb.kind == 'cmds'
            S._put_cmds(bw, mb, last, s, rng, st)
    return S.Built(bw.bytes(), st, bytes(s.out), False)


def one(lgwin, cmds, name=''):
    return S.Stream(lgwin, [S.MB('cmds', cmds=cmds)], name)


# ---------------------------------------------------------------- the decoder's cases
DICT = bytes((i * 37 + 11) % 251 for i in range(97))   # 97 distinct bytes: every address tells


def decoder_cases():
    """[(name, Stream, dictionary)]: compound copies at every placement the rule distinguishes"""
    L, out = len(DICT), []

    def d(pos, a, lgwin=16):
        return ('dist', distance_of(pos, lgwin, L, a))
    out.append(('address_0', one(16, [(b'ab', 5, d(2, 0)), (b'.', 2, None)])))
    out.append(('middle', one(16, [(b'ab', 10, d(2, 40)), (b'.', 2, None)])))
    out.append(('ends_on_last_byte', one(16, [(b'ab', 6, d(2, L - 6)), (b'.', 2, None)])))
    out.append(('one_past_the_end', one(16, [(b'ab', 7, d(2, L - 6)), (b'.', 2, None)])))
    out.append(('whole_dictionary', one(16, [(b'ab', L, d(2, 0)), (b'.', 2, None)])))
    out.append(('ends_the_metablock', one(16, [(b'xy', 8, d(2, 10))])))
    # distance code 0 after a dictionary copy: the same distance from a position 5 bytes on is
    # the address 5 bytes on -- the run goes on; and it pushes again
    out.append(('then_code_0', one(16, [(b'ab', 5, d(2, 3)), (b'', 4, ('short', 0)), (b'c', 3, ('dist', 2)), (b'.', 2, None)])))
    out.append(('then_implicit', one(16, [(b'ab', 5, d(2, 3)), (b'q', 4, ('implicit',)), (b'r', 6, ('short', 1)),
                                          (b'.', 2, None)])))
    # short codes around a dictionary distance: ring[0] - 1 is one address further on
    out.append(('then_short_4', one(16, [(b'ab', 5, d(2, 30)), (b'', 5, ('short', 4)), (b'.', 2, None)])))
    lits = bytes((i * 11 + 5) & 0xFF for i in range(1200))
    out.append(('beyond_max_backward', one(10, [(lits, 9, d(1200, 20, 10)), (b'mid', 4, ('short', 0)),
                                                (b'', 12, d(1216, L - 12, 10)), (b'.', 2, None)])))
    # lgwin 10: the decoder's ring is 1,024 bytes.  A copy from the dictionary that crosses the
    # ring's end, and one that ends exactly there, with more of the stream behind them
    out.append(('crosses_the_ring_end', one(10, [(lits[:1000], 60, d(1000, 10, 10)), (b'tail', 5, ('short', 0)),
                                                 (lits[:900], 30, d(1969, 50, 10)), (b'.', 2, None)])))
    out.append(('ends_at_the_ring_end', one(10, [(lits[:1000], 24, d(1000, 70, 10)), (b'more of it', 2, None)])))
    return [(n, s, DICT) for n, s in out]
