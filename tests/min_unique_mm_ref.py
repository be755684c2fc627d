"""Minimum unique length with mismatches over a text, independent of the FM-index: the expected values of dg_min_unique_mm
(include/dicey_gpu.h) and the bedGraph `dicey mappability -u -w` writes.  mul_e(p) is the smallest k in 1..limit(p) at which the
k-mer at p is the only valid window of the text within e substitutions of it and of its reverse complement.  Two models:
  sweep     the definition read aloud: the first k at which the brute-force (k,e)-mappability of tests/mappability_mm_ref.py is 1
            (its `ball` method, so max_k <= 32)
  pairwise  no k at all.  Another window stays within e of the one at p for as long as fewer than e + 1 mismatches have gone by and
            both windows are valid, so every PAIR of starts has one largest length at which it still counts, and mul_e(p) is one more
            than the largest of those over all partners of p.  Same strand: along the diagonal d = q - p the partner of length k is
            the window at p + d; the length ends at the (e+1)-th mismatch of T against T shifted by d, counted from p, at run(p) and at
            run(p + d).  The bound is symmetric in the pair.  Other strand: along the anti-diagonal s the partner of length k is the
            window that ENDS at s - p, read backward and complemented: T[p + j] against the complement of T[s - p - j]; the length ends
            at the (e+1)-th mismatch, at run(p) and at the backward run that ends at s - p.  The window at p itself is one of those
            partners (a k-mer within e of its own reverse complement).
pairwise is quadratic in the text: keep every text under about 8 000 bytes."""
import numpy as np

import mappability_mm_ref as MM
from min_unique_ref import run_lengths

ES = (0, 1, 2)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b
_bounds = {}  # text -> ({e: same-strand bound per position}, {e: other-strand bound per position})
_sweeps = {}


def sweep(text: bytes, max_k: int, e: int, forward_only: bool = False) -> np.ndarray:
    """uint32[len(text)]: the smallest k in 1..max_k with mappability_mm_ref.values(text, k, e)[p] == 1, else 0"""
    assert max_k <= 32
    key = (text, e, bool(forward_only))
    k_done, first = _sweeps.get(key, (0, np.zeros(len(text), dtype=np.uint32)))
    for k in range(k_done + 1, max_k + 1):
        v = MM.values(text, k, e, forward_only=forward_only)
        first[(first == 0) & (v == 1)] = k
        k_done = k
    _sweeps[key] = (k_done, first)
    out = first.copy()
    out[out > max_k] = 0
    return out


def back_run_lengths(text: bytes) -> np.ndarray:
    """int64[len(text)]: the number of consecutive A/C/G/T bytes that END at p"""
    return run_lengths(text[::-1])[::-1].copy()


def _nth_mismatch(neq: np.ndarray, e: int) -> np.ndarray:
    """per index x of neq: the index of the (e+1)-th True at or behind x, len(neq) when there are fewer"""
    mp = np.nonzero(neq)[0]
    far = np.concatenate([mp, np.full(e + 1, len(neq), dtype=mp.dtype)])
    return far[np.searchsorted(mp, np.arange(len(neq))) + e]


def pair_bounds(text: bytes):
    """({e: int64[L]}, {e: int64[L]}): per position the largest length at which ANOTHER window of the same strand, and any window of
    the other strand, is still valid and within e of the window at p (cut at run(p) as well); e in 0, 1, 2"""
    if text in _bounds:
        return _bounds[text]
    t = np.frombuffer(text, dtype=np.uint8)
    L = len(t)
    run, back = run_lengths(text), back_run_lengths(text)
    same = {e: np.zeros(L, dtype=np.int64) for e in ES}
    other = {e: np.zeros(L, dtype=np.int64) for e in ES}
    idx = np.arange(L, dtype=np.int64)
    for d in range(1, L):
        m = L - d  # pairs (p, p + d), p < m
        neq = t[:m] != t[d:]
        cut = np.minimum(run[:m], run[d:])
        for e in ES:
            b = np.minimum(_nth_mismatch(neq, e) - idx[:m], cut)
            np.maximum(same[e][:m], b, out=same[e][:m])
            np.maximum(same[e][d:], b, out=same[e][d:])
    tc = _COMP[t]
    for s in range(2 * L - 1):
        x0, x1 = max(0, s - L + 1), min(L - 1, s)  # positions x with 0 <= s - x < L
        xs = idx[x0:x1 + 1]
        neq = t[x0:x1 + 1] != tc[s - xs]
        cut = np.minimum(run[x0:x1 + 1], back[s - xs])
        for e in ES:
            b = np.minimum(_nth_mismatch(neq, e) - (xs - x0), cut)
            np.maximum(other[e][x0:x1 + 1], b, out=other[e][x0:x1 + 1])
    _bounds[text] = (same, other)
    return _bounds[text]


def pairwise(text: bytes, max_k: int, e: int, forward_only: bool = False) -> np.ndarray:
    """uint32[len(text)]: 1 + the largest bound, 0 where that exceeds limit(p) = min(run(p), max_k) or p is not A/C/G/T"""
    same, other = pair_bounds(text)
    best = same[e] if forward_only else np.maximum(same[e], other[e])
    limit = np.minimum(run_lengths(text), max_k)
    out = best + 1
    out[out > limit] = 0
    return out.astype(np.uint32)


def coverage(text: bytes, max_k: int, e: int) -> dict:
    """what an input exercises at this e, by the reference alone: among positions with mul_{e-1} != 0 those whose length grows and
    those that lose it; among all positions those the other strand raises and those it leaves without a length"""
    both, fwd, below = pairwise(text, max_k, e), pairwise(text, max_k, e, True), pairwise(text, max_k, e - 1)
    had = below != 0
    return {"raised": int((had & (both > below)).sum()), "became_zero": int((had & (both == 0)).sum()),
            "reverse_raises": int((both > fwd).sum()), "reverse_zeroes": int(((fwd != 0) & (both == 0)).sum())}


def bedgraph(text: bytes, names, max_k: int, e: int, forward_only: bool = False) -> bytes:
    """the bytes `dicey mappability -u -w e -k max_k` writes for the genome whose index text is `text` (sequences in FASTA order)"""
    return MM.bedgraph(pairwise(text, max_k, e, forward_only), text, names)


def crafted_seqs(seed: int = 29):
    """the sequences of the crafted genome of tests/test_gpu_min_unique_mm.py, about 5 kb: near-copies on either strand whose mismatches
    are spaced so that one and two of them are outrun at different lengths, partial near-copies that end in an N run and at a sequence
    end (the partner goes invalid before the mismatches run out), a reverse-complement palindrome, the same with one base changed (two
    mismatches against its own reverse complement: the changed base and its mirror image), one of odd length (one mismatch against its
    own reverse complement: the middle base), a poly-A, an IUPAC letter and sequences shorter than every max_k"""
    import random
    from conftest import revcomp
    rng = random.Random(seed)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))

    def every(s, step, first=None):  # another base at every step-th position
        s = list(s)
        for i in range(step - 1 if first is None else first, len(s), step):
            s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        return "".join(s)

    seg, stretch, half = rnd(1200), rnd(120), rnd(14)
    pal = half + revcomp(half)
    pal1 = pal[:5] + {"A": "C", "C": "A", "G": "T", "T": "G"}[pal[5]] + pal[6:]
    s1 = rnd(150) + seg + "A" + rnd(200) + every(seg, 25) + "C" + rnd(150)
    s2 = rnd(100) + every(revcomp(seg[:600]), 17) + rnd(100) + stretch + rnd(80) + every(stretch[:70], 40, 30) + "N" * 12 + rnd(100) + "R" + rnd(60)
    odd = rnd(14)
    odd = odd + "G" + revcomp(odd)
    s3 = rnd(80) + pal + rnd(80) + pal1 + rnd(80) + odd + rnd(80) + "A" * 300 + rnd(80)
    s6 = rnd(150) + every(stretch[20:100], 40, 25)
    return {"seqs": [s1, s2, s3, "ACGTAC", rnd(9), s6], "pal": pal, "pal1": pal1, "odd": odd, "stretch": stretch}
