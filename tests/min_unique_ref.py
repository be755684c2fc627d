"""Minimum unique length over a text, independent of the FM-index: the expected values of dg_min_unique (include/dicey_gpu.h) and the
bedGraph `dicey mappability -u` writes.  Two models:
  by_values  the definition read aloud: the first k at which the brute-force mappability of tests/mappability_ref.py equals 1
  direct     suffixes sorted on their first max_k + 1 bytes, the common prefixes of neighbours, and a substring search for the
             reverse complement"""
import numpy as np

import mappability_ref as R

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_sweeps = {}  # (text, forward_only) -> [k reached, first k with value 1 per position (0: none so far)]


def run_lengths(text: bytes) -> np.ndarray:
    """int64[len(text)]: the number of consecutive A/C/G/T bytes from p"""
    ok = R._CODE[np.frombuffer(text, dtype=np.uint8)] != 255
    L = len(ok)
    idx = np.arange(L, dtype=np.int64)
    nxt = np.where(~ok, idx, L)  # the next position at or behind p that is not A/C/G/T
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    return nxt - idx


def by_values(text: bytes, max_k: int, forward_only: bool = False) -> np.ndarray:
    """uint32[len(text)]: the smallest k in 1..max_k with mappability_ref.values(text, k)[p] == 1, else 0.  (values() is 0 where the
    k-mer leaves the run of A/C/G/T, so the run bounds k by itself.)  The sweep over k is kept per text and extended on demand: the
    answer for a smaller max_k is the same sweep stopped earlier."""
    key = (text, bool(forward_only))
    k_done, first = _sweeps.get(key, (0, np.zeros(len(text), dtype=np.uint32)))
    for k in range(k_done + 1, max_k + 1):
        v = R.values(text, k, forward_only=forward_only)
        first[(first == 0) & (v == 1)] = k
        k_done = k
    _sweeps[key] = (k_done, first)
    out = first.copy()
    out[out > max_k] = 0
    return out


def coverage(text: bytes, max_k: int) -> dict:
    """what an input exercises, by the reference alone: A/C/G/T positions, zeros among them (still repeated at the limit), positions
    whose both-strand value exceeds the forward-only one (the reverse pass raises the forward number), positions the other strand
    keeps at 0, and the smallest value"""
    both, fwd = by_values(text, max_k), by_values(text, max_k, True)
    acgt = run_lengths(text) > 0
    assert not both[~acgt].any() and not fwd[~acgt].any()
    return {"acgt": int(acgt.sum()), "zeros": int((both[acgt] == 0).sum()), "raised": int((both > fwd).sum()),
            "kept_zero": int(((both == 0) & (fwd != 0)).sum()), "smallest": int(both[both > 0].min())}


def monotone(text: bytes, max_k: int, forward_only: bool = False) -> bool:
    """value_{k+1}(p) <= value_k(p) wherever the (k+1)-mer at p is valid, k = 1..max_k-1"""
    prev = R.values(text, 1, forward_only=forward_only)
    for k in range(1, max_k):
        nxt = R.values(text, k + 1, forward_only=forward_only)
        ok = R.valid_positions(text, k + 1)
        if (nxt[ok] > prev[ok]).any():
            return False
        prev = nxt
    return True


def direct(text: bytes, max_k: int, forward_only: bool = False) -> np.ndarray:
    L = len(text)
    t = text + b"\0"  # the sentinel: two different suffixes differ at the latest here
    order = sorted(range(L + 1), key=lambda p: t[p:p + max_k + 1])
    run = run_lengths(text)

    def lcp(a, b):
        j = 0
        while j <= max_k and a + j <= L and b + j <= L and t[a + j] == t[b + j]:
            j += 1
        return j

    out = np.zeros(L, dtype=np.uint32)
    for r, p in enumerate(order):
        if p == L or run[p] == 0:
            continue
        limit = min(int(run[p]), max_k)
        m = 0
        if r > 0:
            m = max(m, lcp(order[r - 1], p))
        if r + 1 <= L:
            m = max(m, lcp(p, order[r + 1]))
        need = m + 1
        if need > limit:
            continue
        if not forward_only:
            k = 1  # the first k at which revcomp(T[p, p+k)) is no substring of the text (a window with N or '\n' never equals one)
            while k <= limit and t.find(t[p:p + k].translate(_COMP)[::-1]) >= 0:
                k += 1
            if k > limit:
                continue
            need = max(need, k)
        out[p] = need
    return out


def bedgraph(text: bytes, names, max_k: int, forward_only: bool = False) -> bytes:
    """the bytes `dicey mappability -u -k max_k` writes for the genome whose index text is `text` (sequences in FASTA order)"""
    vals = by_values(text, max_k, forward_only)
    out = []
    off = 0
    for name, seq in zip(names, text.split(b"\n")[:-1]):
        s, ln, v = R.runs(vals, off, off + len(seq))
        for a, b, c in zip((s - off).tolist(), ln.tolist(), v.tolist()):
            out.append(b"%s\t%d\t%d\t%d\n" % (name.encode(), a, a + b, c))
        off += len(seq) + 1
    return b"".join(out)
