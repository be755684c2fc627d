"""Brute-force (k,e)-mappability over a text, independent of the FM-index: the expected values of dg_mappability_mm
(include/dicey_gpu.h).  value_e(p) = #{valid q : Hamming(T[q,q+k), w) <= e} + the same against revcomp(w), w = T[p,p+k) valid.

Two references that share nothing but the valid-position rule:
  diagonal  any k, any e, texts up to a few tens of kb: for every offset d the per-position inequality of T against T shifted by d
            (and of T against revcomp(T)), window sums from a cumulative sum, pairs of valid windows within e counted;
  ball      k <= 32: valid windows as 2-bit codes, counts of the distinct codes, summed over the XOR-mask Hamming ball.
`direct` is a third, per-position count used for a handful of positions."""
from itertools import combinations, product

import numpy as np

import mappability_ref as R

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def _finish(fwd, rev, forward_only, max_count):
    out = fwd.astype(np.uint64) + (0 if forward_only else rev.astype(np.uint64))
    out = np.minimum(out, 0xFFFFFFFF)
    if max_count:
        out = np.minimum(out, max_count)
    return out.astype(np.uint32)


def parts_diagonal(text: bytes, k: int, es=(0, 1, 2)):
    """{e: (fwd_e, rev_e)} as int64[len(text)] arrays (0 at invalid positions)"""
    t = np.frombuffer(text, dtype=np.uint8)
    L = len(t)
    valid = R.valid_positions(text, k)
    nw = L - k + 1  # window starts 0 .. nw-1
    fwd = {e: np.zeros(L, dtype=np.int64) for e in es}
    rev = {e: np.zeros(L, dtype=np.int64) for e in es}
    if nw <= 0:
        return {e: (fwd[e], rev[e]) for e in es}
    v = valid[:nw]
    # forward: window p against window p + d
    for d in range(nw):
        neq = t[d:] != t[:L - d]
        cs = np.concatenate([[0], np.cumsum(neq, dtype=np.int32)])
        m = nw - d  # pairs (p, p + d), p < m
        ham = cs[k:k + m] - cs[:m]
        both = v[:m] & v[d:d + m]
        for e in es:
            hit = both & (ham <= e)
            fwd[e][:m] += hit
            if d:
                fwd[e][d:d + m] += hit
    # reverse: the window at q, reverse complemented, is the window at nw-1-q of rc = revcomp(T); compare T[p..] with rc[p + d ..]
    rc = _COMP[t][::-1]
    vr = v[::-1]  # validity of rc's window r = validity of T's window nw-1-r
    for d in range(-(nw - 1), nw):
        p0, p1 = max(0, -d), min(nw, nw - d)  # windows p in [p0, p1), partner r = p + d in [0, nw)
        if p1 <= p0:
            continue
        a = t[p0:p1 + k - 1]
        b = rc[p0 + d:p1 + d + k - 1]
        cs = np.concatenate([[0], np.cumsum(a != b, dtype=np.int32)])
        ham = cs[k:] - cs[:len(cs) - k]
        both = v[p0:p1] & vr[p0 + d:p1 + d]
        for e in es:
            rev[e][p0:p1] += both & (ham <= e)
    return {e: (fwd[e], rev[e]) for e in es}


def _masks(k, e):
    out = [0]
    for r in range(1, e + 1):
        for pos in combinations(range(k), r):
            for xs in product((1, 2, 3), repeat=r):
                m = 0
                for p, x in zip(pos, xs):
                    m |= x << (2 * p)
                out.append(m)
    return np.array(out, dtype=np.uint64)


def parts_ball(text: bytes, k: int, e: int):
    """(fwd_e, rev_e) as int64[len(text)] arrays, k <= 32"""
    assert k <= 32
    L = len(text)
    valid = R.valid_positions(text, k)
    pos = np.nonzero(valid)[0]
    fwd = np.zeros(L, dtype=np.int64)
    rev = np.zeros(L, dtype=np.int64)
    if not len(pos):
        return fwd, rev
    c = R._CODE[np.frombuffer(text, dtype=np.uint8)].astype(np.uint64)
    c[c == 255] = 0
    fw = np.zeros(len(pos), dtype=np.uint64)
    rc = np.zeros(len(pos), dtype=np.uint64)
    for j in range(k):
        cj = c[pos + j]
        fw = (fw << np.uint64(2)) | cj
        rc |= (np.uint64(3) - cj) << np.uint64(2 * j)
    keys, inv, cnt = np.unique(fw, return_inverse=True, return_counts=True)
    rkeys, rinv = np.unique(rc, return_inverse=True)
    cnt = cnt.astype(np.int64)

    def look(q):
        ix = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
        return np.where(keys[ix] == q, cnt[ix], 0)

    sf = np.zeros(len(keys), dtype=np.int64)
    sr = np.zeros(len(rkeys), dtype=np.int64)
    for m in _masks(k, e):
        sf += look(keys ^ m)
        sr += look(rkeys ^ m)
    fwd[pos] = sf[inv]
    rev[pos] = sr[rinv]
    return fwd, rev


def values(text: bytes, k: int, e: int, forward_only: bool = False, max_count: int = 0, method: str = "ball") -> np.ndarray:
    """uint32[len(text)] = value_e of every position"""
    fwd, rev = parts_ball(text, k, e) if method == "ball" else parts_diagonal(text, k, (e,))[e]
    return _finish(fwd, rev, forward_only, max_count)


def direct(text: bytes, k: int, e: int, positions, forward_only: bool = False):
    """value_e of a few positions, each by comparing its k-mer with every window of the text"""
    t = np.frombuffer(text, dtype=np.uint8)
    valid = R.valid_positions(text, k)
    nw = len(t) - k + 1
    win = np.lib.stride_tricks.sliding_window_view(t, k)[:nw][valid[:nw]]
    out = []
    for p in positions:
        if not valid[p]:
            out.append(0)
            continue
        w = t[p:p + k]
        n = int(((win != w).sum(axis=1) <= e).sum())
        if not forward_only:
            n += int(((win != _COMP[w][::-1]).sum(axis=1) <= e).sum())
        out.append(n)
    return np.array(out, dtype=np.int64)


def bedgraph(vals: np.ndarray, text: bytes, names) -> bytes:
    """the bytes `dicey mappability` writes for these values (sequences of `text` in FASTA order)"""
    out = []
    off = 0
    for name, seq in zip(names, text.split(b"\n")[:-1]):
        s, ln, v = R.runs(vals, off, off + len(seq))
        for a, b, c in zip((s - off).tolist(), ln.tolist(), v.tolist()):
            out.append(b"%s\t%d\t%d\t%d\n" % (name.encode(), a, a + b, c))
        off += len(seq) + 1
    return b"".join(out)
