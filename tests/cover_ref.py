"""Per-base tracks over a text, independent of the FM-index: the expected values of dg_map_cover and dg_map_min_cover
(include/dicey_gpu.h) and the bedGraph `dicey mappability -p` writes.  Two models of each track:
  cover                 a cumulative sum over the start-position values it is given
  cover_by_windows      the definition read aloud: every specific k-mer of tests/mappability_ref.py / mappability_mm_ref.py adds one
                        to each base it lies over
  min_cover             the formula over a length array: min over starts q of max(mul(q), p-q+1) inside q's run
  min_cover_by_windows  every (q, m) with value_m(q) == 1 walked directly: the bases of that window are covered at length m"""
import random

import numpy as np

import mappability_mm_ref as MM
import mappability_ref as R
from min_unique_ref import run_lengths


def cover(base_values: np.ndarray, k: int, at_most: int = 1, max_count: int = 0) -> np.ndarray:
    """uint32[L]: the number of starts q in max(0, p-k+1) .. p with 1 <= base_values[q] <= at_most; min(., max_count) when max_count > 0"""
    v = np.asarray(base_values).astype(np.int64)
    spec = (v >= 1) & (v <= at_most)
    cs = np.concatenate([[0], np.cumsum(spec, dtype=np.int64)])
    p = np.arange(len(v), dtype=np.int64)
    out = cs[p + 1] - cs[np.maximum(p - k + 1, 0)]
    if max_count:
        out = np.minimum(out, max_count)
    return out.astype(np.uint32)


def _values(text, k, e, forward_only):
    if e == 0:
        return R.values(text, k, forward_only=forward_only)
    return MM.values(text, k, e, forward_only=forward_only, method="ball" if k <= 32 else "diagonal")


def cover_by_windows(text: bytes, k: int, at_most: int = 1, max_count: int = 0, e: int = 0, forward_only: bool = False) -> np.ndarray:
    v = _values(text, k, e, forward_only).astype(np.int64)
    out = np.zeros(len(text), dtype=np.int64)
    for q in np.nonzero((v >= 1) & (v <= at_most))[0].tolist():
        out[q:q + k] += 1  # (a specific k-mer is valid: it lies inside the text)
    if max_count:
        out = np.minimum(out, max_count)
    return out.astype(np.uint32)


def min_cover(text: bytes, mul: np.ndarray, max_k: int) -> np.ndarray:
    """uint32[L]: min{max(mul(q), p-q+1) : p-max_k+1 <= q <= p, q >= 0, mul(q) != 0, run(q) >= p-q+1}, 0 when the set is empty"""
    L = len(text)
    mul = np.asarray(mul).astype(np.int64)
    run = run_lengths(text)
    big = 1 << 40
    best = np.full(L, big, dtype=np.int64)
    for d in range(1, min(max_k, L) + 1):
        q = np.arange(0, L - d + 1)  # p = q + d - 1
        ok = (mul[q] != 0) & (run[q] >= d)
        cand = np.where(ok, np.maximum(mul[q], d), big)
        best[d - 1:] = np.minimum(best[d - 1:], cand)
    best[best == big] = 0
    return best.astype(np.uint32)


def min_cover_by_windows(text: bytes, max_k: int, e: int = 0, forward_only: bool = False) -> np.ndarray:
    """uint32[L]: the smallest m in 1..max_k such that some start q has value_m(q) == 1 and q <= p < q + m, 0 when there is none"""
    L = len(text)
    out = np.zeros(L, dtype=np.uint32)
    for m in range(1, max_k + 1):
        one = (_values(text, m, e, forward_only) == 1).astype(np.int64)
        cs = np.concatenate([[0], np.cumsum(one)])
        p = np.arange(L, dtype=np.int64)
        over = (cs[p + 1] - cs[np.maximum(p - m + 1, 0)]) > 0
        out[over & (out == 0)] = m
    return out


def coverable(text: bytes, k: int) -> np.ndarray:
    """bool[L]: the base lies in at least one valid k-window"""
    return cover(R.valid_positions(text, k).astype(np.uint32), k) > 0


def bedgraph(vals: np.ndarray, text: bytes, names) -> bytes:
    """the bytes `dicey mappability -p` writes for these per-base values (sequences of `text` in FASTA order)"""
    return MM.bedgraph(vals, text, names)


def crafted_seqs(seed: int = 41):
    """about 1.6 kb: a 300 bp repeat on both strands, a 20-mer reverse-complement palindrome, N runs that cut A/C/G/T runs of 15 and 30
    bases out, sequences of 6 and 12 bases, a 150 bp poly-A and an R"""
    rng = random.Random(seed)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    comp = str.maketrans("ACGT", "TGCA")
    rep = rnd(300)
    half = rnd(10)
    pal = half + half.translate(comp)[::-1]
    s1 = rnd(120) + rep + rnd(60) + "NNN" + rnd(15) + "NN" + rnd(30) + "N" + rnd(80) + pal + rnd(50)
    s2 = rnd(6)
    s3 = rnd(90) + rep.translate(comp)[::-1] + rnd(40) + "R" + rnd(70) + "A" * 150 + rnd(45)
    s4 = rnd(12)
    s5 = rnd(35) + rep[100:180] + rnd(25)
    return [s1, s2, s3, s4, s5]
