"""Histograms chosen to reach the edge paths of a prefix code's construction and serialisation
(createHuffmanTree's count-limit retry, the simple forms, the run-length codes' corner cases),
for the tests that compare the encoder's Huffman kernel with the reference's
buildAndStoreHuffmanTree (tests/test_gpu_prefix_codes.py) and the host test that proves, on the
reference alone, that they reach what they claim (tests/test_entropy_audit_host.py).

A case is (name, histogram); the histogram's length is its alphabet: 256 (literal), 704
(command) or 64 (distance)."""
import numpy as np

ALPHABETS = (256, 704, 64)
ZERO_RUNS = (1, 2, 3, 10, 11, 12, 138, 139, 300)
DEPTH_RUNS = (1, 2, 3, 4, 5, 6, 7, 8, 11, 70)


def fibonacci(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def powers_of_two(n):
    return [1 << i for i in range(n)]


def scattered(counts, alphabet, seed):
    """the counts at seeded positions over the whole alphabet, in a seeded order"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(alphabet, size=len(counts), replace=False))
    h = [0] * alphabet
    for p, c in zip(pos, rng.permutation(counts)):
        h[int(p)] = int(c)
    return h


def packed(counts, alphabet):
    """the counts on the alphabet's last symbols"""
    return [0] * (alphabet - len(counts)) + list(counts)


def at(alphabet, pairs):
    h = [0] * alphabet
    for s, c in pairs:
        h[s] = c
    return h


def zero_runs(runs, alphabet):
    """used symbols (all different counts) with these runs of unused symbols between them, and
    four more used symbols after the last (the complex form needs five); None when it does not fit"""
    need = sum(runs) + len(runs) + 5
    if need > alphabet:
        return None
    h, p = [0] * alphabet, 0
    for k, r in enumerate(runs):
        h[p] = 3 + 5 * k
        p += 1 + r
    for j in range(5):
        h[p + j] = 7 + 2 * j
    return h


def _dyadic(depths):
    """counts 2^(max - depth): Huffman code lengths of a dyadic law are its -log2 p, whatever the ties"""
    top = max(d for d in depths if d)
    return [(1 << (top - d)) if d else 0 for d in depths]


def depth_run(run, alphabet):
    """a histogram whose code has `run` neighbouring symbols of one length d, then single symbols
    of other lengths with an unused symbol between them; None when it does not fit"""
    d = 3
    while (1 << d) <= run:
        d += 1
    depths = [d] * run
    rest = (1 << d) - run   # the Kraft sum left, in units of 2^-d
    fill = [d - b for b in range(rest.bit_length() - 1, -1, -1) if (rest >> b) & 1]
    while run + len(fill) < 6:   # more than four used symbols: split the deepest
        fill = fill[:-1] + [fill[-1] + 1] * 2
    for f in fill:
        depths += [0, f]
    if len(depths) > alphabet:
        return None
    return _dyadic(depths + [0] * (alphabet - len(depths)))


def crafted(alphabet):
    """the chosen cases of one alphabet"""
    a, last = alphabet, alphabet - 1
    out = [('none used', [0] * a),
           ('one used: symbol 0', at(a, [(0, 9)])),
           ('one used: the last symbol', at(a, [(last, 1)])),
           ('two used, equal', at(a, [(3, 5), (last, 5)])),
           ('two used', at(a, [(0, 1), (17, 1000)])),
           ('three used, equal', at(a, [(1, 2), (2, 2), (40, 2)])),
           ('three used', at(a, [(5, 100), (6, 1), (last, 10)])),
           ('three used, the first the rarest', at(a, [(0, 1), (30, 7), (31, 7)])),
           ('four used: 2,2,2,2', at(a, [(0, 5), (9, 5), (33, 5), (last, 5)])),
           ('four used: 2,2,2,2 by unequal counts', at(a, [(2, 3), (3, 4), (50, 5), (51, 6)])),
           ('four used: 1,2,3,3', at(a, [(4, 1), (12, 8), (13, 2), (63, 4)])),
           ('four used: 1,2,3,3, deepest first', at(a, [(0, 1), (1, 1), (2, 2), (last, 4)])),
           ('five used', at(a, [(0, 1), (1, 1), (2, 1), (3, 1), (last, 1)])),
           ('five used, skewed', at(a, [(7, 1), (8, 50), (20, 3), (21, 1000), (last - 1, 9)]))]
    for name, counts in (('fibonacci 16', fibonacci(16)), ('fibonacci 17', fibonacci(17)),
                         ('fibonacci 32', fibonacci(32)), ('powers of two 18', powers_of_two(18))):
        out.append((name + ', scattered', scattered(counts, a, len(counts))))
        out.append((name + ', packed at the end', packed(counts, a)))
    out.append(('all %d used, equal' % a, [3] * a))
    if a > 256:
        out.append(('the first 256 used, equal', [7] * 256 + [0] * (a - 256)))
    fit = [r for r in ZERO_RUNS if r < a]
    one = zero_runs(fit, a)
    if one is not None:
        out.append(('zero runs %s' % (fit,), one))
    else:   # in pieces: as many runs a histogram as fit
        while fit:
            n = len(fit)
            while zero_runs(fit[:n], a) is None:
                n -= 1
            out.append(('zero runs %s' % (fit[:n],), zero_runs(fit[:n], a)))
            fit = fit[n:]
    for r in DEPTH_RUNS:
        h = depth_run(r, a)
        if h is not None:
            out.append(('equal-depth run of %d' % r, h))
    out.append(('2^24 among thirty ones', scattered([1 << 24] + [1] * 30, a, 24)))
    return out


def random_histograms(alphabet, n, seed):
    """seeded histograms of mixed sparsity and count laws; totals stay far below 2^32"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        used = max(1, int(alphabet * rng.choice([0.01, 0.03, 0.1, 0.3, 0.6, 1.0])))
        used = min(alphabet, int(rng.integers(1, used + 1)) if rng.random() < 0.3 else used)
        law = int(rng.integers(0, 4))
        if law == 0:
            c = rng.integers(1, 8, size=used)                       # small counts, many ties
        elif law == 1:
            c = np.floor(2.0 ** (rng.random(used) * 20)).astype(np.int64)   # log-uniform up to 2^20
        elif law == 2:
            c = np.maximum(1, (1e6 / np.arange(1, used + 1) ** 1.3)).astype(np.int64)   # Zipf-like
            c = rng.permutation(c)
        else:
            c = np.floor(rng.exponential(300.0, size=used)).astype(np.int64) + 1
        if rng.random() < 0.5:   # a contiguous range (long equal / zero runs), else scattered
            start = int(rng.integers(0, alphabet - used + 1))
            pos = np.arange(start, start + used)
        else:
            pos = np.sort(rng.choice(alphabet, size=used, replace=False))
        h = [0] * alphabet
        for p, v in zip(pos, c):
            h[int(p)] = int(v)
        out.append(('random %d/%d' % (alphabet, k), h))
    return out


def runs_of(values):
    """[(value, run length)] of a sequence"""
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(v, n) for v, n in out]
