"""Input generators shared by the encoder's tests: inputs built to reach more than four block
types per category, and the literal path's stress input."""
import numpy as np

from brotli_amd import datagen


def eight_alphabets(n=65536):
    """eight pieces of n bytes over different alphabets: one metablock of them gets more than four
    literal block types (block-splitter.ts:15,359: up to 256 types)"""
    nxt = datagen.xorshift32(77)

    def over(alpha):
        return bytes(alpha[nxt() % len(alpha)] for _ in range(n))
    pieces = [datagen.enwik_text(n, 31), datagen.glyf_stream(n, 32), over(b'ACGT'), over(b'0123456789abcdef'),
              over(b'ABCDEFGHIJKLMNOPQRSTUVWXYZ234567'), over(b' .,;:!?-'), over(bytes(range(128, 192))),
              bytes(48 + (i * 7 + (i >> 5)) % 10 for i in range(n))]
    return b''.join(pieces)


def kinds_input(seed=5, n=65536):
    """eight 64 KiB pieces whose commands differ in kind: no copies, runs, short periods, two
    record strides, text, copies from far back, short-alphabet data"""
    nxt = datagen.xorshift32(seed)
    rnd = bytes(nxt() & 0xFF for _ in range(n))
    runs = b''.join(bytes([nxt() & 0xFF]) * (4 + nxt() % 60) for _ in range(n // 20))[:n]
    period = bytes((i % 3) * 40 + (nxt() % 2) for i in range(n))

    def records(stride):
        out = bytearray(rnd[:stride])
        while len(out) < n:
            r = bytearray(out[len(out) - stride:])
            r[nxt() % stride] = nxt() & 0xFF
            out += r
        return bytes(out[:n])
    text = datagen.enwik_text(n, seed + 1)
    far = bytes(b ^ (1 if nxt() % 97 == 0 else 0) for b in text)
    dna = bytes(b'ACGT'[nxt() % 4] for _ in range(n))
    return b''.join([rnd, runs, period, records(48), text, records(1000), far, dna])


def lit_stress(n, seed):
    """skewed bytes over all 256 values with a different law after each class of previous byte,
    literal runs of 1-200 bytes and runs of short copies between them (the decoder's literal
    path, tests/test_gpu_literal_tables.py)"""
    rng = np.random.default_rng(seed)
    # per class of the previous byte (p1 >> 6), a Zipf-like law over a permutation whose most
    # likely values lie in the next class: the contexts predict very different bytes
    draws = []   # per class: pre-drawn bytes of its law, taken in order
    for k in range(4):
        nxt = (k + 1) & 3
        own = rng.permutation(np.arange(64 * nxt, 64 * nxt + 64))
        rest = rng.permutation(np.setdiff1d(np.arange(256), own))
        perm = np.concatenate([own, rest])
        w = 1.0 / np.arange(1, 257) ** (0.8 + 0.15 * k)
        cdf = np.cumsum(w / w.sum())
        draws.append(perm[np.minimum(255, np.searchsorted(cdf, rng.random(n)))].tolist())
    at = [0, 0, 0, 0]
    out = bytearray()
    prev = 0
    while len(out) < n:
        run = int(rng.integers(1, 200))
        for _ in range(run):
            k = prev >> 6
            prev = draws[k][at[k]]
            at[k] += 1
            out.append(prev)
        if len(out) > 64:
            for _ in range(int(rng.integers(0, 5))):   # a run of copies
                ln = int(rng.integers(4, 48))
                d = int(rng.integers(1, 64)) if rng.random() < 0.3 else int(rng.integers(64, len(out)))
                d = min(d, len(out))
                for _ in range(ln):
                    out.append(out[len(out) - d])
                prev = out[-1]
    return bytes(out[:n])
