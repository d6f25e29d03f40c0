"""An RFC 7932 stream WRITER for the decoder's tests, and a plain model of what such a stream decodes to.

Written from RFC 7932 alone (sections 3-10); pure Python, nothing imported from brotli_amd.
A stream is DESCRIBED (Stream / MB below): the window, the metablocks, and for a compressed
metablock its commands, block splits, context maps and the SHAPE of every prefix code -- so a
test states which header features and how many table entries a stream has instead of hoping an
encoder produces them.  build() serialises a description; model() applies the same command
list with plain byte copies (overlapping copies byte by byte) and needs no decoder.

Static-dictionary word references: the writer knows the LENGTH of a transformed word for the six
transforms of WORD_DELTA only, and never its bytes -- restating the 121 transforms in Python is
out of scope.  For a stream with word references model() returns None and the expected bytes
come from the oracle alone; such a stream uses one literal tree, so no literal context depends
on bytes the writer does not know.

Table sizes are controlled, not guessed: a code whose lengths are all <= 8 occupies exactly
256 entries of a decoder's two-level table (root 8 bits), a single-symbol code too; a code with
one chain of longer lengths ending at length m adds one second-level block of 2^(m - 8)
entries.  table_size() restates that count; placed_mb() solves a metablock's total from it.

One alignment is avoided on purpose: a metadata metablock with MSKIPBYTES > 0 whose header ends
exactly on a byte boundary (decoders of the Java lineage read one bit more there than RFC 9.2
says); meta blocks at that alignment are written with MSKIPBYTES = 0 instead.
"""
import random

INS_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]
INS_BITS = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
COPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
COPY_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
BLEN_BASE = [1, 5, 9, 13, 17, 25, 33, 41, 49, 65, 81, 97, 113, 145, 177, 209, 241, 305, 369, 497, 753, 1265, 2289,
             4337, 8433, 16625]
BLEN_BITS = [2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24]
# section 5: (insert code >> 3, copy code >> 3) -> first command code of the cell, explicit distance
CELL = {(0, 0): 128, (0, 1): 192, (0, 2): 384, (1, 0): 256, (1, 1): 320, (1, 2): 512, (2, 0): 448, (2, 1): 576,
        (2, 2): 640}
CELL_IMPLICIT = {(0, 0): 0, (0, 1): 64}
CL_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]
CL_FIXED = {0: (0b00, 2), 1: (0b0111, 4), 2: (0b011, 3), 3: (0b10, 2), 4: (0b01, 2), 5: (0b1111, 4)}
SHORT_IDX = [0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
SHORT_DELTA = [0, 0, 0, 0, -1, 1, -2, 2, -3, 3, -1, 1, -2, 2, -3, 3]
NDBITS = [0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5]
# transform id -> change of length: Identity, Identity+" ", " "+Identity+" ", OmitFirst1, UppercaseFirst, OmitLast1
WORD_DELTA = {0: 0, 1: 1, 2: 2, 3: -1, 9: 0, 12: -1}
LSB6, MSB6, UTF8, SIGNED = 0, 1, 2, 3

LUT0 = ([0] * 9 + [4, 4, 0, 0, 4, 0, 0] + [0] * 16 +
        [8, 12, 16, 12, 12, 20, 12, 16, 24, 28, 12, 12, 32, 12, 36, 12] +
        [44] * 10 + [32, 32, 24, 40, 28, 12] +
        [12, 48, 52, 52, 52, 48, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48] +
        [52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 24, 12, 28, 12, 12] +
        [12, 56, 60, 60, 60, 56, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56] +
        [60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 24, 12, 28, 12, 0] +
        [0, 1] * 32 + [2, 3] * 32)
LUT1 = ([0] * 32 + [0] + [1] * 15 + [2] * 10 + [1] * 6 + [1] + [2] * 26 + [1] * 5 + [1] + [3] * 26 + [1, 1, 1, 1, 0] +
        [0] * 64 + [0] * 32 + [2] * 32)
LUT2 = [0] + [1] * 15 + [2] * 48 + [3] * 64 + [4] * 64 + [5] * 48 + [6] * 15 + [7]
assert len(LUT0) == len(LUT1) == len(LUT2) == 256


def context(mode, p1, p2):
    """section 7.1: the literal context id from the last two bytes"""
    if mode == LSB6:
        return p1 & 63
    if mode == MSB6:
        return p1 >> 2
    if mode == UTF8:
        return LUT0[p1] | LUT1[p2]
    return (LUT2[p1] << 3) | LUT2[p2]


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.k = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n), (v, n)
        self.acc |= v << self.k
        self.k += n
        while self.k >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.k -= 8

    def bitpos(self):
        return len(self.buf) * 8 + self.k

    def align(self):
        if self.k:
            self.put(0, 8 - self.k)

    def raw(self, data):
        assert self.k == 0
        self.buf += data

    def bytes(self):
        self.align()
        return bytes(self.buf)


def put_varlen(bw, v):
    """the 1..256 code of NBLTYPES / NTREES (section 9.2), v = value - 1"""
    if v == 0:
        bw.put(0, 1)
        return
    bw.put(1, 1)
    n = v.bit_length() - 1
    bw.put(n, 3)
    bw.put(v - (1 << n), n)


# ---------------------------------------------------------------- prefix codes
def balanced(k):
    """lengths of a complete code over k symbols, as flat as possible"""
    if k == 1:
        return [0]
    top = (k - 1).bit_length()
    short = (1 << top) - k
    return [top - 1] * short + [top] * (k - short)


def lengths_for(used, alphabet, depth=None, rng=None, pad=0):
    """{symbol: length} of a complete code that contains `used` (padded with unused symbols to
    `pad`), flat, and with one chain down to `depth` when depth exceeds the flat code's length."""
    syms = sorted(used)
    spare = [x for x in range(alphabet) if x not in used]
    if rng is not None:
        rng.shuffle(spare)
    while len(syms) < max(2, pad):
        syms.append(spare.pop())
    if rng is not None:
        rng.shuffle(syms)
    lens = dict(zip(syms, balanced(len(syms))))
    b = max(lens.values())
    if depth is not None and depth > b:
        assert depth - b <= len(spare), 'no unused symbols left for the chain'
        lens[syms[-1]] = min(b + 1, depth)
        for ln in list(range(b + 2, depth)) + ([depth] if depth > b + 1 else []) + [depth]:
            lens[spare.pop()] = ln
    assert sum(1 << (15 - v) for v in lens.values()) == 1 << 15, lens
    return lens


def table_size(lens):
    """entries of the two-level lookup table (root 8 bits) a decoder builds for these lengths"""
    count = [0] * 16
    for v in lens.values():
        count[v] += 1
    count[0] = 0
    if sum(count) == 1:
        return 256

    def next_key(key, ln):
        step = 1 << (ln - 1)
        while key & step:
            step >>= 1
        return (key & (step - 1)) + step
    key, total, low = 0, 256, -1
    for ln in range(1, 16):
        while count[ln]:
            if ln > 8 and (key & 255) != low:
                b, left = ln, 1 << (ln - 8)
                while b < 15:
                    left -= count[b]
                    if left <= 0:
                        break
                    b += 1
                    left <<= 1
                total += 1 << (b - 8)
                low = key & 255
            key = next_key(key, ln)
            count[ln] -= 1
    return total


def _canon(lens):
    """section 3.2: {symbol: (bit-reversed code, length)}"""
    enc, code = {}, 0
    for ln in range(1, 16):
        for s in sorted(x for x in lens if lens[x] == ln):
            enc[s] = (int(format(code, '0%db' % ln)[::-1], 2), ln)
            code += 1
        code <<= 1
    if len(lens) == 1:
        enc[next(iter(lens))] = (0, 0)
    return enc


def _bijective(x, base):
    d = []
    while x > 0:
        r = x % base or base
        d.append(r)
        x = (x - r) // base
    return d[::-1]


class Code:
    """one prefix code: its lengths, and how its description is written (section 3.4 simple,
    3.5 complex with HSKIP and the repeat codes 16 / 17)"""

    def __init__(self, lens, alphabet, simple=None, rle=True):
        self.lens, self.alphabet, self.simple, self.rle = lens, alphabet, simple, rle
        self.enc = _canon(lens)
        self.size = table_size(lens)

    def put(self, bw, sym):
        bw.put(*self.enc[sym])

    def write(self, bw, st):
        if self.simple is not None:
            order, select = self.simple
            bw.put(1, 2)
            bw.put(len(order) - 1, 2)
            for s in order:
                bw.put(s, max(1, (self.alphabet - 1).bit_length()))
            if len(order) == 4:
                bw.put(select, 1)
            st['nsym'].add(len(order))
            st['tree_select'].add((len(order), select))
            return
        flat = [self.lens.get(i, 0) for i in range(max(self.lens) + 1)]
        cl = []   # (code length symbol, extra value, extra bits)
        i = 0
        while i < len(flat):
            v, j = flat[i], i
            while j < len(flat) and flat[j] == v:
                j += 1
            run = j - i
            if v:
                cl.append((v, 0, 0))
                run -= 1
            if self.rle and run >= 3:
                for d in _bijective(run - 2, 4 if v else 8):
                    cl.append((16 if v else 17, d - 1, 2 if v else 3))
                st['rep16' if v else 'rep17'] += 1
                if run - 2 > (4 if v else 8):
                    st['rep_chained'] += 1
            else:
                cl += [(v, 0, 0)] * run
            i = j
        st['maxlen'] = max(st['maxlen'], max(flat))
        hist = {}
        for s, _, _ in cl:
            hist[s] = hist.get(s, 0) + 1
        by_freq = sorted(hist, key=lambda s: (-hist[s], s))
        cl_lens = dict(zip(by_freq, balanced(len(by_freq))))
        if len(by_freq) == 1:
            cl_lens[by_freq[0]] = 3   # a lone code length code: any length, zero bits per symbol
        skip = 0
        while cl_lens.get(CL_ORDER[skip], 0) == 0:
            skip += 1
        skip = 3 if skip >= 3 else 2 if skip == 2 else 0
        st['hskip'].add(skip)
        bw.put(skip, 2)
        space = 32
        for s in CL_ORDER[skip:]:
            v = cl_lens.get(s, 0)
            bw.put(*CL_FIXED[v])
            if v:
                space -= 32 >> v
                if space <= 0 and len(by_freq) > 1:
                    break
        enc = _canon(cl_lens) if len(by_freq) > 1 else {by_freq[0]: (0, 0)}
        for s, e, n in cl:
            bw.put(*enc[s])
            bw.put(e, n)


def make_code(used, alphabet, shape, rng, st):
    """shape: {'depth': m or None, 'simple': bool, 'pad': n, 'select': 0/1, 'rle': bool, 'sorted': bool}"""
    depth = shape.get('depth')
    pad = shape.get('pad', 0)
    if (depth is None or depth <= 8) and len(used) <= 4 and max(len(used), pad, 1) <= 4 and shape.get('simple', True):
        order = sorted(used)
        spare = (x for x in range(alphabet) if x not in used)
        while len(order) < max(1, pad):
            order.append(next(spare))
        n, select = len(order), shape.get('select', 0)
        ln = {1: [0], 2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if select else [2, 2, 2, 2]}[n]
        if rng is not None and not shape.get('sorted'):   # ('sorted': the symbols stay in ascending order)
            rng.shuffle(order)
        return Code(dict(zip(order, ln)), alphabet, simple=(order, select))
    return Code(lengths_for(used, alphabet, depth, rng, pad), alphabet, rle=shape.get('rle', True))


# ---------------------------------------------------------------- descriptions
class MB:
    """one metablock.  kind 'cmds': commands = [(insert bytes, copy length, distance spec)], the
    spec one of ('implicit',), ('short', code 0..15), ('dist', d), ('word', index, transform) or
    None (the last command, whose insert ends the metablock).  kind 'raw': data.  kind 'meta':
    data (skipped).  kind 'empty': ISLAST + ISLASTEMPTY."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.data = b''
        self.mnibbles = None          # None: the smallest that holds MLEN
        self.cmds = []
        self.ntypes = [1, 1, 1]
        self.blocks = [None, None, None]   # per category [('first', n), ('prev' | 'next' | type, n), ...]
        self.npostfix, self.ndirect = 0, 0   # ndirect: the 4-bit field (NDIRECT >> NPOSTFIX)
        self.modes = [0]
        self.lmap, self.ntrees_l, self.lmap_rle, self.lmap_imtf = [0] * 64, 1, 0, False
        self.dmap, self.ntrees_d, self.dmap_rle, self.dmap_imtf = [0] * 4, 1, 0, False
        self.shapes = {}              # (group, tree) -> shape of make_code; group 'L' 'I' 'D' 'BT0'.. 'BC0'.. 'LM' 'DM'
        self.__dict__.update(kw)


class Stream:
    def __init__(self, lgwin, mbs, name='', seed=0):
        self.lgwin, self.mbs, self.name, self.seed = lgwin, mbs, name, seed


class State:
    """what a decoder knows between commands: the output so far and the last four distances"""

    def __init__(self, lgwin):
        self.lgwin, self.out, self.ring, self.words = lgwin, bytearray(), [4, 11, 15, 16], False

    def maxd(self):
        return min(len(self.out), (1 << self.lgwin) - 16)

    def resolve(self, spec, copy_len):
        """(distance, distance code or None, pushes the ring, output length)"""
        if spec[0] == 'implicit':
            return self.ring[0], None, False, copy_len
        if spec[0] == 'short':
            return self.ring[SHORT_IDX[spec[1]]] + SHORT_DELTA[spec[1]], spec[1], spec[1] != 0, copy_len
        if spec[0] == 'dist':
            return spec[1], -1, True, copy_len
        _, index, transform = spec
        assert 4 <= copy_len <= 24 and index < (1 << NDBITS[copy_len])
        return self.maxd() + 1 + index + (transform << NDBITS[copy_len]), -1, False, copy_len + WORD_DELTA[transform]

    def copy(self, spec, copy_len):
        d, code, push, n = self.resolve(spec, copy_len)
        if spec[0] == 'word':
            self.out += b'?' * n
            self.words = True
            return d, code
        assert 0 < d <= self.maxd(), (spec, d, self.maxd())
        for _ in range(n):
            self.out.append(self.out[-d])
        if push:
            self.ring = [d] + self.ring[:3]
        return d, code


def model(stream):
    """the decoded bytes by plain copies, or None when the stream has word references"""
    out, ring = bytearray(), [4, 11, 15, 16]
    for mb in stream.mbs:
        if mb.kind == 'raw':
            out += mb.data
        for ins, n, spec in (mb.cmds if mb.kind == 'cmds' else []):
            out += ins
            if spec is None:
                continue
            if spec[0] == 'word':
                return None
            if spec[0] == 'implicit':
                d = ring[0]
            elif spec[0] == 'short':
                d = ring[SHORT_IDX[spec[1]]] + SHORT_DELTA[spec[1]]
            else:
                d = spec[1]
            if spec not in (('implicit',), ('short', 0)):
                ring = [d] + ring[:3]
            for _ in range(n):
                out.append(out[len(out) - d])
    return bytes(out)


def _code_of(base, v):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c, v - base[c]


def _dist_code(d, npostfix, ndirect):
    """section 4: (distance code, extra value, extra bits) of an explicit distance"""
    if d <= ndirect:
        return 15 + d, 0, 0
    x = d - ndirect - 1
    lcode, q = x & ((1 << npostfix) - 1), (x >> npostfix) + 4
    nbits = q.bit_length() - 2
    half = (q >> nbits) & 1
    return 16 + ndirect + (((2 * (nbits - 1) + half) << npostfix) | lcode), q - ((2 + half) << nbits), nbits


class _Blocks:
    def __init__(self, plan, ntypes, cat, ev, st):
        self.plan, self.n, self.cat, self.ev, self.st = plan, ntypes, cat, ev, st
        self.i, self.type, self.prev = 0, 0, 1
        self.left = plan[0][1] if ntypes > 1 else 1 << 28

    def step(self):
        if self.left == 0:
            self.i += 1
            how, length = self.plan[self.i]
            sym, t = (0, self.prev) if how == 'prev' else (1, self.type + 1) if how == 'next' else (how + 2, how)
            self.st['switch'].add(min(sym, 2))
            if t >= self.n:
                t -= self.n
                self.st['type_wrap'] += 1
            self.prev, self.type = self.type, t
            self.ev(('sym', 'BT%d' % self.cat, 0, sym))
            c, e = _code_of(BLEN_BASE, length)
            self.ev(('sym', 'BC%d' % self.cat, 0, c))
            self.ev(('bits', e, BLEN_BITS[c]))
            self.left = length
        self.left -= 1


def _walk(mb, s, ev, st):
    """the metablock's commands as the sequence of symbols and extra bits a decoder reads"""
    bl = [_Blocks(mb.blocks[c], mb.ntypes[c], c, ev, st) for c in range(3)]
    ndirect = mb.ndirect << mb.npostfix
    for k, (ins, n, spec) in enumerate(mb.cmds):
        bl[1].step()
        ic, ie = _code_of(INS_BASE, len(ins))
        cc, ce = _code_of(COPY_BASE, n)
        implicit = spec is not None and spec[0] == 'implicit'
        base = (CELL_IMPLICIT if implicit else CELL)[(ic >> 3, cc >> 3)]
        ev(('sym', 'I', bl[1].type, base | ((ic & 7) << 3) | (cc & 7)))
        ev(('bits', ie, INS_BITS[ic]))
        ev(('bits', ce, COPY_BITS[cc]))
        st['cells'].add(base)
        for b in ins:
            bl[0].step()
            t = bl[0].type
            p1 = s.out[-1] if s.out else 0
            p2 = s.out[-2] if len(s.out) > 1 else 0
            ev(('sym', 'L', mb.lmap[t * 64 + context(mb.modes[t], p1, p2)], b))
            st['modes_used'].add(mb.modes[t])
            s.out.append(b)
        if spec is None:
            assert k == len(mb.cmds) - 1
            continue
        pos = len(s.out)
        d, code, _, outn = s.resolve(spec, n)
        if not implicit:
            bl[2].step()
            if code == -1:
                code, e, nb = _dist_code(d, mb.npostfix, ndirect)
                st['direct' if nb == 0 else 'postfix'] += 1
            else:
                e, nb = 0, 0
                st['short'].add(code)
            ev(('sym', 'D', mb.dmap[bl[2].type * 4 + min(n, 5) - 2], code))
            ev(('bits', e, nb))
        else:
            st['implicit'] += 1
        s.copy(spec, n)
        if spec[0] == 'word':
            st['words'] += 1
            continue
        if n > 64:
            st['long_copy'] += 1
        if d < n:
            st['overlap'].add(d)
        if s.lgwin == 10 and (pos >> 10) != ((pos + n - 1) >> 10):
            st['ring_cross'] += 1


def _put_map(bw, cmap, ntrees, rlemax, imtf, shape, rng, st):
    """section 7.3: a context map"""
    put_varlen(bw, ntrees - 1)
    if ntrees == 1:
        assert not any(cmap)
        return
    vals = list(cmap)
    if imtf:
        mtf = list(range(256))
        for i, v in enumerate(vals):
            j = mtf.index(v)
            vals[i] = j
            mtf.insert(0, mtf.pop(j))
    syms, i = [], 0
    while i < len(vals):
        if vals[i]:
            syms.append((vals[i] + rlemax, 0, 0))
            i += 1
            continue
        j = i
        while j < len(vals) and vals[j] == 0:
            j += 1
        run = j - i
        while run:
            c = min(rlemax, run.bit_length() - 1)
            if c == 0:
                syms.append((0, 0, 0))
                run -= 1
            else:
                reps = min(run, (2 << c) - 1)
                syms.append((c, reps - (1 << c), c))
                run -= reps
        i = j
    bw.put(1 if rlemax else 0, 1)
    if rlemax:
        bw.put(rlemax - 1, 4)
    code = make_code({x[0] for x in syms}, ntrees + rlemax, shape, rng, st)
    code.write(bw, st)
    for sy, e, n in syms:
        code.put(bw, sy)
        bw.put(e, n)
    bw.put(1 if imtf else 0, 1)
    st['map_rle'] += 1 if rlemax else 0
    st['map_plain'] += 0 if rlemax else 1
    st['map_imtf'] += 1 if imtf else 0
    st['map_no_imtf'] += 0 if imtf else 1


def _put_cmds(bw, mb, last, s, rng, st):
    ev = []
    start = len(s.out)
    _walk(mb, s, ev.append, st)
    mlen = len(s.out) - start
    assert mlen > 0
    used = {}
    for e in ev:
        if e[0] == 'sym':
            used.setdefault((e[1], e[2]), set()).add(e[3])
    for c in range(3):   # the first block count of each category is in the header
        if mb.ntypes[c] > 1:
            used.setdefault(('BC%d' % c, 0), set()).add(_code_of(BLEN_BASE, mb.blocks[c][0][1])[0])
    nib = mb.mnibbles or max(4, ((mlen - 1).bit_length() + 3) // 4)
    assert nib in (4, 5, 6) and (mlen - 1) < (1 << (4 * nib)) and (nib == 4 or (mlen - 1) >> (4 * nib - 4))
    st['mnibbles'].add(nib)
    bw.put(1 if last else 0, 1)
    if last:
        bw.put(0, 1)
    bw.put(nib - 4, 2)
    bw.put(mlen - 1, 4 * nib)
    if not last:
        bw.put(0, 1)
    ndist = 16 + (mb.ndirect << mb.npostfix) + (48 << mb.npostfix)
    alphabets = {'L': 256, 'I': 704, 'D': ndist}
    codes = {}

    def code(group, tree):
        a = alphabets.get(group) or (26 if group[:2] == 'BC' else mb.ntypes[int(group[2])] + 2)
        codes[group, tree] = make_code(used.get((group, tree), set()), a, mb.shapes.get((group, tree), {}), rng, st)
        codes[group, tree].write(bw, st)
        return codes[group, tree]
    for c in range(3):
        put_varlen(bw, mb.ntypes[c] - 1)
        if mb.ntypes[c] > 1:
            code('BT%d' % c, 0)
            bc = code('BC%d' % c, 0)
            n, e = _code_of(BLEN_BASE, mb.blocks[c][0][1])
            bc.put(bw, n)
            bw.put(e, BLEN_BITS[n])
    bw.put(mb.npostfix, 2)
    bw.put(mb.ndirect, 4)
    st['npostfix'].add(mb.npostfix)
    st['ndirect'].add(mb.ndirect)
    assert len(mb.modes) == mb.ntypes[0] and len(mb.lmap) == 64 * mb.ntypes[0] and len(mb.dmap) == 4 * mb.ntypes[2]
    assert max(mb.lmap) < mb.ntrees_l and max(mb.dmap) < mb.ntrees_d
    for m in mb.modes:
        bw.put(m, 2)
    _put_map(bw, mb.lmap, mb.ntrees_l, mb.lmap_rle, mb.lmap_imtf, mb.shapes.get(('LM', 0), {}), rng, st)
    _put_map(bw, mb.dmap, mb.ntrees_d, mb.dmap_rle, mb.dmap_imtf, mb.shapes.get(('DM', 0), {}), rng, st)
    total = mb.ntrees_l + mb.ntypes[1] + mb.ntrees_d
    for group, n in (('L', mb.ntrees_l), ('I', mb.ntypes[1]), ('D', mb.ntrees_d)):
        for t in range(n):
            total += code(group, t).size
    st['totals'].append(total)
    st['trees_used'] |= {k for k in used if k[0] in 'LID'}
    for e in ev:
        if e[0] == 'sym':
            codes[e[1], e[2]].put(bw, e[3])
        else:
            bw.put(e[1], e[2])


class Built:
    def __init__(self, data, stats, out, words):
        self.data, self.stats, self.sim_out, self.words = data, stats, out, words


def new_stats():
    st = {k: 0 for k in ('rep16', 'rep17', 'rep_chained', 'maxlen', 'type_wrap', 'implicit', 'direct', 'postfix',
                         'words', 'long_copy', 'ring_cross', 'map_rle', 'map_plain', 'map_imtf', 'map_no_imtf',
                         'raw_mid', 'meta_mid')}
    st.update({k: set() for k in ('nsym', 'tree_select', 'hskip', 'switch', 'cells', 'modes_used', 'short', 'overlap',
                                  'mnibbles', 'npostfix', 'ndirect', 'trees_used', 'skipbytes')})
    st['totals'] = []
    return st


def build(stream):
    """serialise a description: Built(data, stats, the writer's own output, has words)"""
    bw, st, s = BitWriter(), new_stats(), State(stream.lgwin)
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
        elif mb.kind == 'raw':
            assert not last and mb.data
            n = len(mb.data) - 1
            nib = mb.mnibbles or max(4, (n.bit_length() + 3) // 4)
            assert nib == 4 or n >> (4 * nib - 4)
            bw.put(0, 1)
            bw.put(nib - 4, 2)
            bw.put(n, 4 * nib)
            bw.put(1, 1)
            bw.align()
            bw.raw(mb.data)
            s.out += mb.data
            st['raw_mid'] += 1 if k else 0
            st['mnibbles'].add(nib)
        elif mb.kind == 'meta':
            assert not last
            nbytes = max(1, ((len(mb.data) - 1).bit_length() + 7) // 8) if mb.data else 0
            data = mb.data
            if nbytes and (bw.bitpos() + 6 + 8 * nbytes) % 8 == 0:   # the avoided alignment (module docstring)
                nbytes, data = 0, b''
            assert (len(data) == 0) == (nbytes == 0)
            bw.put(0, 1)
            bw.put(3, 2)
            bw.put(0, 1)
            bw.put(nbytes, 2)
            if nbytes:
                assert len(data) - 1 < (1 << (8 * nbytes)) and (nbytes == 1 or (len(data) - 1) >> (8 * nbytes - 8))
                bw.put(len(data) - 1, 8 * nbytes)
            bw.align()
            bw.raw(data)
            st['meta_mid'] += 1 if k else 0
            st['skipbytes'].add(nbytes)
        else:
            _put_cmds(bw, mb, last, s, rng, st)
    assert not (s.words and any(mb.kind == 'cmds' and mb.ntrees_l > 1 for mb in stream.mbs))
    return Built(bw.bytes(), st, bytes(s.out), s.words)


# ---------------------------------------------------------------- generators
def split_blocks(rng, count, ntypes, style='mixed', first=None, sizes=(1, 2, 3, 7, 20, 60)):
    """a block plan that covers `count` symbols of a category with `ntypes` block types"""
    if ntypes == 1:
        return None
    plan, left = [('first', min(count, first or rng.randint(1, max(1, count // 3))))], count
    left -= plan[0][1]
    while left > 0:
        n = min(left, rng.choice(sizes) if style == 'mixed' else 1)
        how = rng.choice(['prev', 'next', 'next', rng.randrange(ntypes)]) if style == 'mixed' else style
        plan.append((how, n))
        left -= n
    return plan


def gen_cmds(rng, s, ncmds, alphabet, words=False, dmax=None, long_every=9, end_insert=True):
    """random commands, valid against the state s (which they are applied to)"""
    cmds = []
    for k in range(ncmds):
        r = rng.random()
        n_ins = 0 if r < 0.25 and s.out else rng.randint(1, 8) if r < 0.85 else rng.choice([9, 17, 40, 70, 140])
        ins = bytes(rng.choice(alphabet) for _ in range(n_ins))
        s.out += ins
        n = rng.choice([2, 3, 4, 5, 6, 8, 9, 11, 13, 17, 25, 33, 60])
        if k % long_every == long_every - 1:
            n = rng.choice([65, 70, 101, 140, 200, 330, 600])
        maxd = s.maxd() if dmax is None else min(s.maxd(), dmax)
        spec = None
        for _ in range(8):
            r = rng.random()
            if words and r < 0.2:
                n = rng.randint(4, 24)
                cand = ('word', rng.randrange(1 << NDBITS[n]), rng.choice(sorted(WORD_DELTA)))
            elif r < 0.25 and len(ins) < 6 and n < 70:
                cand = ('implicit',)
            elif r < 0.5:
                cand = ('short', rng.randrange(16))
            elif r < 0.62:
                cand = ('dist', rng.choice([1, 2, 3, 63]))
            elif r < 0.8:
                cand = ('dist', rng.randint(1, min(maxd, 140)))
            else:
                cand = ('dist', rng.randint(1, maxd))
            if cand[0] == 'word' or 0 < s.resolve(cand, n)[0] <= maxd:
                spec = cand
                break
        if spec is None:
            spec = ('dist', 1)
        s.copy(spec, n)
        cmds.append((ins, n, spec))
    if end_insert:
        tail = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 5)))
        s.out += tail
        cmds.append((tail, 2, None))
    return cmds


def count_symbols(cmds):
    return (sum(len(c[0]) for c in cmds), len(cmds),
            sum(1 for c in cmds if c[2] is not None and c[2][0] != 'implicit'))


def solve_total(total):
    """(number of trees, chain depths) of a metablock whose three groups total `total` entries:
    each tree costs its root and 256 entries, a chain to depth m another 2^(m - 8)"""
    n = total // 257
    while True:
        rem = total - 257 * n
        depths = []
        if rem % 2 == 0:
            for d in range(7, 0, -1):
                while rem >= (1 << d) and not (d < 7 and depths.count(8 + d)):
                    depths.append(8 + d)
                    rem -= 1 << d
            if rem == 0 and len(depths) <= n:
                return n, depths
        n -= 1
        assert n >= 3, total


def placed_mb(rng, s, total, n_cmd_trees=3, n_dist_trees=9, ncmds=40, literals=None, words=False):
    """a compressed metablock whose tree groups total exactly `total` table entries, whose
    commands reach the LAST literal, command and distance tree, each with symbols of its own"""
    n, depths = solve_total(total)
    n_cmd_trees = min(n_cmd_trees, max(1, n - 2))
    n_dist_trees = n - n_cmd_trees - 1 if words else min(n_dist_trees, max(1, n - n_cmd_trees - 1))
    nl = n - n_cmd_trees - n_dist_trees
    if nl > 256:
        n_dist_trees += nl - 256
        nl = 256
    assert 1 <= nl and n_dist_trees <= 256
    if words:
        assert nl == 1
    literals = literals or bytes(range(48, 112))
    mb = MB('cmds')
    mb.ntypes = [(nl + 63) // 64, n_cmd_trees, (n_dist_trees + 3) // 4]
    mb.npostfix, mb.ndirect = rng.randrange(4), rng.randrange(16)
    mb.modes = [LSB6] * mb.ntypes[0]
    mb.ntrees_l, mb.ntrees_d = nl, n_dist_trees
    mb.lmap = [k % nl for k in range(64 * mb.ntypes[0])]
    mb.dmap = [k % n_dist_trees for k in range(4 * mb.ntypes[2])]
    mb.lmap[-1], mb.dmap[-1] = nl - 1, n_dist_trees - 1
    mb.lmap_rle, mb.dmap_rle = (rng.choice([0, 3, 16]), rng.choice([0, 2])) if nl > 1 else (0, 0)
    mb.lmap_imtf, mb.dmap_imtf = rng.random() < 0.5, rng.random() < 0.5
    # commands: the tail goes through the last block type of every category, with a literal in
    # context 63, a copy of length >= 5 (distance context 3) at an explicit distance
    mb.cmds = gen_cmds(rng, s, ncmds, literals, words=words, end_insert=False)
    tail = [(b'\x3f' + bytes([literals[1]]) + b'\x7f' + bytes([literals[2]]), 7, ('dist', len(s.out) + 4 - 1)),
            (b'\x3f' + bytes([literals[3]]), 9, ('dist', 2)), (bytes([literals[5]]), 2, None)]
    for ins, cn, spec in tail:
        s.out += ins
        if spec:
            s.copy(spec, cn)
    ntail = count_symbols(tail)
    counts = count_symbols(mb.cmds)
    mb.cmds += tail
    for c in range(3):
        if mb.ntypes[c] > 1:
            assert counts[c] > 0
            mb.blocks[c] = split_blocks(rng, counts[c], mb.ntypes[c], first=max(1, counts[c] // 4))
            mb.blocks[c].append((mb.ntypes[c] - 1, ntail[c] + 3))
    # the chains: distance and command trees first (large alphabets), then literal trees
    slots = [('D', t) for t in range(n_dist_trees - 1, -1, -1)] + [('I', t) for t in range(n_cmd_trees - 1, -1, -1)] + \
            [('L', t) for t in range(nl - 1, -1, -1)]
    for k, d in enumerate(depths):
        mb.shapes[slots[k]] = {'depth': d, 'rle': k % 2 == 0}
    mb.want_total = total
    return mb


def placed(total, lgwin=18, seed=1, **kw):
    rng = random.Random(seed)
    s = State(lgwin)
    return Stream(lgwin, [placed_mb(rng, s, total, **kw)], 'placed_%d' % total, seed)


def lit256(seed=2):
    """256 literal codes of at most 8 bits, one command code, one distance code: 66,306 entries,
    literal tree 255's root at 65,536 and every later root beyond 16 bits"""
    st = placed(256 + 256 * 256 + 257 + 257, seed=seed, n_cmd_trees=1, n_dist_trees=1)
    st.name = 'lit256'
    return st


def transitions(seed=3, lgwin=17):
    """small tables, raw, large tables (beyond every LDS cap), metadata, small tables again"""
    rng = random.Random(seed)
    s = State(lgwin)
    a = placed_mb(rng, s, 2500, ncmds=25)
    raw = bytes(rng.randrange(256) for _ in range(37))
    s.out += raw
    b = placed_mb(rng, s, 70000, ncmds=25)
    c = placed_mb(rng, s, 9000, ncmds=25)
    raw2 = bytes(rng.randrange(256) for _ in range(5))
    s.out += raw2
    d = placed_mb(rng, s, 13000, ncmds=20)
    e = placed_mb(rng, s, 1100, ncmds=20)
    return Stream(lgwin, [a, MB('raw', data=raw), b, MB('meta', data=b'skip me' * 9), c, MB('raw', data=raw2),
                          MB('meta', data=b''), d, e, MB('empty')], 'transitions', seed)


def long_run(mlen, lgwin=22):
    """MNIBBLES 5 / 6: one literal and copies at distance 1 up to mlen bytes"""
    cmds, left = [], mlen - 1
    ins = b'r'
    while left > 0:
        n = min(left, 2118 + (1 << 24) - 1)
        if 0 < left - n < 2:
            n -= 2
        cmds.append((ins, n, ('dist', 1) if not cmds else ('short', 0)))
        ins, left = b'', left - n
    return Stream(lgwin, [MB('cmds', cmds=cmds)], 'long_run_%d' % mlen)


def many_types(seed=4, lgwin=16):
    """256 block types in every category; the literal blocks step through all of them with
    symbol 1 and wrap past NBLTYPES"""
    rng = random.Random(seed)
    s = State(lgwin)
    mb = MB('cmds')
    mb.cmds = gen_cmds(rng, s, 150, b'abcdefgh\x3f\xff\x00')
    nlit, ncmd, ndist = count_symbols(mb.cmds)
    mb.ntypes = [256, 256, 256]
    mb.modes = [t & 3 for t in range(256)]
    mb.ntrees_l, mb.lmap = 7, [(k * 5 + (k >> 6)) % 7 for k in range(64 * 256)]
    mb.ntrees_d, mb.dmap = 5, [(k * 3) % 5 for k in range(4 * 256)]
    mb.lmap_rle, mb.lmap_imtf, mb.dmap_imtf = 6, True, True
    mb.blocks = [split_blocks(rng, nlit, 256, style='next', first=1), split_blocks(rng, ncmd, 256, first=1, sizes=(1, 2, 3)),
                 split_blocks(rng, ndist, 256, style='next', first=2)]
    assert nlit > 300
    return Stream(lgwin, [mb], 'many_types', seed)


def ring_wrap(seed=5):
    """lgwin 10: 1 KiB ring, copies that cross its end, at the largest distance too"""
    rng = random.Random(seed)
    s = State(10)
    mb = MB('cmds')
    mb.cmds = gen_cmds(rng, s, 12, b'wxyz0123', end_insert=False)
    while len(s.out) < 3300:
        fill = 1024 - (len(s.out) & 1023)
        ins = bytes(rng.choice(b'wxyz0123') for _ in range(max(0, fill - 20)))
        s.out += ins
        spec = ('dist', rng.choice([s.maxd(), 1, 2, 3, 63, 1008 if s.maxd() >= 1008 else 1]))
        s.copy(spec, 70)
        mb.cmds.append((ins, 70, spec))
    s.out += b'!'
    mb.cmds.append((b'!', 2, None))
    return Stream(10, [mb], 'ring_wrap', seed)


def word_refs(seed=6, lgwin=20):
    """static-dictionary words of every length, with the six transforms whose length is known"""
    rng = random.Random(seed)
    s = State(lgwin)
    mb = MB('cmds')
    mb.cmds = []
    for n in range(4, 25):
        for t in (0, rng.choice(sorted(WORD_DELTA))):
            ins = bytes(rng.choice(b' ,.') for _ in range(rng.randrange(3)))
            s.out += ins
            spec = ('word', rng.randrange(1 << NDBITS[n]), t)
            s.copy(spec, n)
            mb.cmds.append((ins, n, spec))
    mb.cmds += gen_cmds(rng, s, 30, b' etaoin', words=True)
    return Stream(lgwin, [mb], 'word_refs', seed)


def windows():
    """every window-bits code, lgwin 10..24, on a tiny stream; and the empty stream"""
    out = [Stream(w, [MB('cmds', cmds=[(b'window %d' % w, 4, ('dist', 3)), (b'.', 2, None)])], 'lgwin_%d' % w)
           for w in range(10, 25)]
    out.append(Stream(22, [MB('empty')], 'empty'))
    out.append(Stream(16, [MB('raw', data=b'raw first'), MB('meta', data=b''), MB('empty')], 'raw_first'))
    return out


def meta_sizes():
    """metadata metablocks with MSKIPBYTES 0..3 between compressed ones"""
    mbs = [MB('cmds', cmds=[(b'abc', 3, ('dist', 2)), (b'd', 2, None)])]
    for n in (0, 1, 200, 256, 300, 65536, 65537 + 11):
        mbs.append(MB('meta', data=bytes(range(256)) * (n // 256) + bytes(n % 256)))
        mbs.append(MB('cmds', cmds=[(b'm%d' % n, 4, ('short', 0)), (b'e', 2, None)]))
    return Stream(18, mbs + [MB('empty')], 'meta_sizes')


def simple_codes():
    """NSYM 1..4 and both tree-select shapes in the literal, command and distance codes"""
    mbs = []
    for nsym, select in ((1, 0), (2, 0), (3, 0), (4, 0), (4, 1)):
        lits = b'pqrs'[:nsym]
        cmds = [(lits, 2, ('dist', 1))] + [(lits[k % nsym:k % nsym + 1], 2, ('dist', 1 + k % nsym)) for k in range(8)]
        mb = MB('cmds', cmds=cmds + [(lits[:1], 2, None)])
        shape = {'pad': nsym, 'select': select}
        mb.shapes = {('L', 0): shape, ('I', 0): shape, ('D', 0): shape}
        mbs.append(mb)
    return Stream(12, mbs, 'simple_codes')


BOUNDARIES = (12224, 12225, 65536, 65537, 68096, 68097)


def named():
    """the named streams: placements on both sides of each boundary, and the edges"""
    out = [placed(t, seed=10 + k) for k, t in enumerate(BOUNDARIES)]
    out += [placed(899, seed=20, n_cmd_trees=1, n_dist_trees=1), placed(30000, seed=21), placed(90000, seed=22),
            lit256(), transitions(), long_run(65536 + 70), long_run((1 << 20) + 5), many_types(), ring_wrap(),
            word_refs(), meta_sizes(), simple_codes()]
    w = placed(40000, seed=23, words=True, n_cmd_trees=60)
    w.name = 'placed_words_40000'
    out.append(w)
    return out + windows()


def random_stream(seed):
    """a seeded description: every header feature drawn from explicit parameters"""
    rng = random.Random(seed)
    lgwin = rng.choice([10, 10, 11, 12, 14, 16, 17, 18, 22, 24])
    s = State(lgwin)
    mbs = []
    words = rng.random() < 0.15
    for k in range(rng.randint(1, 4)):
        r = rng.random()
        if r < 0.15:
            data = bytes(rng.randrange(256) for _ in range(rng.randint(1, 90)))
            s.out += data
            mbs.append(MB('raw', data=data))
            continue
        if r < 0.3:
            mbs.append(MB('meta', data=bytes(rng.randrange(256) for _ in range(rng.choice([0, 0, 1, 40, 256, 257, 700])))))
            continue
        mb = MB('cmds')
        alphabet = bytes(rng.sample(range(256), rng.choice([1, 2, 3, 4, 9, 40, 120])))
        mb.cmds = gen_cmds(rng, s, rng.randint(3, 45), alphabet, words=words, end_insert=rng.random() < 0.7)
        counts = count_symbols(mb.cmds)
        mb.ntypes = [rng.choice([1, 2, 3, 5, 9]), rng.choice([1, 2, 4]), rng.choice([1, 2, 3, 7])]
        mb.blocks = [split_blocks(rng, max(1, counts[c]), mb.ntypes[c]) for c in range(3)]
        mb.npostfix, mb.ndirect = rng.randrange(4), rng.randrange(16)
        mb.modes = [rng.randrange(4) for _ in range(mb.ntypes[0])]
        mb.ntrees_l = 1 if words else rng.choice([1, 2, 3, 6, 17])
        mb.lmap = [rng.randrange(mb.ntrees_l) if rng.random() < 0.5 else 0 for _ in range(64 * mb.ntypes[0])]
        mb.ntrees_d = rng.randint(1, min(6, 4 * mb.ntypes[2]))
        mb.dmap = [rng.randrange(mb.ntrees_d) for _ in range(4 * mb.ntypes[2])]
        mb.lmap_rle, mb.dmap_rle = rng.choice([0, 1, 4, 16]), rng.choice([0, 0, 2])
        mb.lmap_imtf, mb.dmap_imtf = rng.random() < 0.5, rng.random() < 0.5
        for g, n in (('L', mb.ntrees_l), ('I', mb.ntypes[1]), ('D', mb.ntrees_d)):
            for t in range(n):
                mb.shapes[g, t] = {'depth': rng.choice([None, None, None, 9, 10, 12, 13, 15]), 'rle': rng.random() < 0.7,
                                   'simple': rng.random() < 0.8, 'pad': rng.choice([0, 0, 2, 3, 4]),
                                   'select': rng.randrange(2)}
        mbs.append(mb)
    if not mbs or mbs[-1].kind != 'cmds' or rng.random() < 0.3:
        mbs.append(MB('empty'))
    return Stream(lgwin, mbs, 'random_%d' % seed, seed)


def random_set(n=200):
    return [random_stream(1000 + k) for k in range(n)]


_corpus = None


def corpus():
    """[(stream, Built)] of every named stream and the seeded set, built once per process"""
    global _corpus
    if _corpus is None:
        _corpus = [(st, build(st)) for st in named() + random_set()]
    return _corpus
