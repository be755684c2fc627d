"""Brute-force query minimum length by END position, independent of the FM-index: the expected values of dg_query_min_len_end
(include/dicey_gpu.h).  For a record Q and a position p, the oligo's LAST base: brun(p) = the consecutive A/C/G/T bytes that end at p
(0 when Q[p] is none; a record start ends a run), limit(p) = min(brun(p), max_k); len(p) = INVALID when limit(p) < min_k, else the
smallest k in [min_k, limit(p)] with value_k(p) <= t, else 0, where value_k(p) is query_anchor_ref's anchored value of the k-mer at
p - k + 1 (the last a bases of the oligo exact on either strand).

`parts_by_k` takes the per-k anchored parts of query_anchor_ref (`ball`: k <= 32; `diagonal`: any k) and shifts them by k - 1 to the
position of the k-mer's last base.  `min_len_end` is a LINEAR SCAN over k that takes the first k whose value is at most t: it does not
bisect and does not assume that values fall with k, so a search bug or a monotonicity bug of the product shows against it.
`violations_by_end` counts the places where the per-k values by end position do rise (the monotonicity argument says: none), `brun_lengths`
reads the runs off the bytes, `bedgraph` writes what `dicey mappability -q -l -E` writes and `record_set` is the set of query shapes the
tests of the feature share.  Parts are kept per (text, buffer, k, e, anchors, route): every test module of one session scans the same ones."""
import numpy as np

import query_anchor_ref as A
import query_map_ref as Q

INVALID = Q.INVALID
_ACGT = np.zeros(256, dtype=bool)
_ACGT[list(b"ACGT")] = True
_PARTS = {}


def brun_lengths(qbuf: bytes):
    """brun(p) for every position of the buffer, from the bytes"""
    ok = _ACGT[np.frombuffer(qbuf, dtype=np.uint8)]
    run = np.zeros(len(qbuf), dtype=np.int64)
    n = 0
    for p in range(len(qbuf)):
        n = n + 1 if ok[p] else 0
        run[p] = n
    return run


def _to_end(arr, k, fill):
    """arr indexed by the k-mer's first base -> indexed by its last base"""
    out = np.full(len(arr), fill, dtype=arr.dtype)
    if len(arr) >= k:
        out[k - 1:] = arr[:len(arr) - k + 1]
    return out


def parts_by_k(text: bytes, qbuf: bytes, ks, e: int, anchors, route: str = "ball"):
    """{k: {a: (fwd, rev, valid)}} by END position: computed once per (k, e), shared across a, t and forward_only.  Anchors above k are
    left out of that k (the entry point takes a <= min_k only)"""
    out = {}
    for k in ks:
        use = tuple(sorted(a for a in set(anchors) if a <= k))
        key = (hash(text), len(text), hash(qbuf), len(qbuf), k, use, route)
        if key + (e,) not in _PARTS:
            if route == "ball":
                by_start = {(e, a): p for a, p in A.parts_ball(text, qbuf, k, e, list(use)).items()}
            else:
                by_start = A.parts_diagonal(text, qbuf, k, (0, 1, 2), list(use))  # (one pass over the shifts serves every e)
            for (ee, a), (f, r, v) in by_start.items():
                _PARTS.setdefault(key + (ee,), {})[a] = (_to_end(f, k, 0), _to_end(r, k, 0), _to_end(v, k, False))
        out[k] = _PARTS[key + (e,)]
    return out


def min_len_end(parts, qbuf: bytes, min_k: int, max_k: int, a: int = 0, t: int = 0, forward_only: bool = False):
    """uint32 per buffer position, from parts_by_k's per-k values: the first k of a linear scan whose value is <= t"""
    assert 0 <= a <= min_k <= max_k
    brun = brun_lengths(qbuf)
    limit = np.minimum(brun, max_k)
    out = np.where(limit < min_k, INVALID, 0).astype(np.uint32)
    todo = limit >= min_k
    for k in range(min_k, max_k + 1):
        fwd, rev, valid = parts[k][a]
        assert (valid == (brun >= k)).all()  # the two validity rules (a k-mer starts at p - k + 1; a run of k ends at p) agree
        v = fwd if forward_only else fwd + rev
        hit = todo & (limit >= k) & (v <= t)
        out[hit] = k
        todo &= ~hit
    return out


def violations_by_end(parts, min_k: int, max_k: int, a: int = 0, forward_only: bool = False):
    """positions and lengths at which the value of the (k+1)-mer that ends at p exceeds that of the k-mer that ends there"""
    bad = 0
    for k in range(min_k, max_k):
        f0, r0, _ = parts[k][a]
        f1, r1, v1 = parts[k + 1][a]
        x, y = (f0, f1) if forward_only else (f0 + r0, f1 + r1)
        bad += int((y[v1] > x[v1]).sum())
    return bad


def split(vals, records):
    return Q.split(vals, records)


def bedgraph(vals_per_record, names) -> bytes:
    """the bytes `dicey mappability -q -l -E` writes: one line per maximal run of equal lengths at the coordinates of the oligo's last base
    (the index of the value); 0 (no length) and INVALID have no line"""
    out = []
    for name, v in zip(names, vals_per_record):
        v = [int(x) for x in v]
        a = 0
        while a < len(v):
            b = a + 1
            while b < len(v) and v[b] == v[a]:
                b += 1
            if v[a] != INVALID and v[a] != 0:
                out.append(("%s\t%d\t%d\t%d\n" % (name, a, b, v[a])).encode())
            a = b
    return b"".join(out)


def record_set(seqs, min_k: int = 10, max_k: int = 24):
    """query_anchor_ref.record_set (its first record lies at buffer offset 0, starts with A/C/G/T and is longer than max_k; its last is kept
    last) and, in front of the last record, the shapes at which the backward limit can go wrong: a record of exactly min_k bytes, a record
    whose A/C/G/T run fills one 64-bit word of the position bitmap exactly (it starts at bit 0 and ends at bit 63, an N behind it), and a
    record whose run of 200 starts at bit 40 of a word and so spans more than three; list of bytes"""
    base = A.record_set(seqs)
    s1, s2, s3 = seqs
    assert len(base[0]) > max_k and _ACGT[list(base[0][:40])].all()
    head, last = base[:-1], base[-1]
    x = A._clean(s2, 12000, min_k)
    head.append(s2[x:x + min_k].encode())
    at = sum(len(r) + 1 for r in head)
    w = A._clean(s3, 24000, 100)
    head.append(("N" * (-at % 64) + A._subst_every(s3[w:w + 64], 23) + "N" + s3[w + 64:w + 100]).encode())
    at = sum(len(r) + 1 for r in head)
    y = A._clean(s1, 26000, 200)
    head.append(("N" * ((40 - at) % 64) + A._subst_every(s1[y:y + 200], 23)).encode())
    return head + [last]
