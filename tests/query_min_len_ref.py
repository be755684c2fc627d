"""Brute-force query minimum length, independent of the FM-index: the expected values of dg_query_min_len (include/dicey_gpu.h).
For a record Q and a position p: run(p) = the consecutive A/C/G/T bytes from p, limit(p) = min(run(p), max_k); len(p) = INVALID when
limit(p) < min_k, else the smallest k in [min_k, limit(p)] with value_k(p) <= t, else 0, where value_k is query_map_ref's.

`min_len` is a LINEAR SCAN over k of the per-k brute-force values (query_map_ref.parts_ball, k <= 32) that takes the first k whose
value is at most t.  It does not bisect and does not assume that values fall with k: a search bug or a monotonicity bug of the product
shows against it.  `violations` counts the places where the per-k values do rise.  `min_len_dict` is a second, unrelated route at e = 0
for any k: the k-mers of the text and of its reverse complement as byte strings, counted in a dict.  `bedgraph` writes what
`dicey mappability -q -l` writes.  `record_set` is the set of query shapes the tests of the feature share."""
import random
from collections import Counter

import numpy as np

import mappability_ref as R
import query_map_ref as Q

INVALID = Q.INVALID
_ACGT = np.zeros(256, dtype=bool)
_ACGT[list(b"ACGT")] = True
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def run_lengths(qbuf: bytes):
    """run(p) for every position of the buffer"""
    ok = _ACGT[np.frombuffer(qbuf, dtype=np.uint8)]
    run = np.zeros(len(qbuf) + 1, dtype=np.int64)
    for p in range(len(qbuf) - 1, -1, -1):
        run[p] = run[p + 1] + 1 if ok[p] else 0
    return run[:-1]


def parts_by_k(text: bytes, qbuf: bytes, ks, e: int):
    """{k: (fwd_e, rev_e, valid)}: computed once per (k, e), shared across t and forward_only"""
    return {k: Q.parts_ball(text, qbuf, k, e) for k in ks}


def min_len(parts, qbuf: bytes, min_k: int, max_k: int, t: int = 0, forward_only: bool = False):
    """uint32 per buffer position, from parts_by_k's per-k values: the first k of a linear scan whose value is <= t"""
    limit = np.minimum(run_lengths(qbuf), max_k)
    out = np.where(limit < min_k, INVALID, 0).astype(np.uint32)
    todo = limit >= min_k
    for k in range(min_k, max_k + 1):
        fwd, rev, valid = parts[k]
        assert (valid == (run_lengths(qbuf) >= k)).all()
        v = fwd if forward_only else fwd + rev
        hit = todo & (limit >= k) & (v <= t)
        out[hit] = k
        todo &= ~hit
    return out


def violations(parts, min_k: int, max_k: int, forward_only: bool = False):
    """positions and lengths at which the value of the (k+1)-mer exceeds that of the k-mer (monotonicity says: none)"""
    bad = 0
    for k in range(min_k, max_k):
        f0, r0, _ = parts[k]
        f1, r1, v1 = parts[k + 1]
        a, b = (f0, f1) if forward_only else (f0 + r0, f1 + r1)
        bad += int((b[v1] > a[v1]).sum())
    return bad


def min_len_dict(text: bytes, qbuf: bytes, min_k: int, max_k: int, t: int = 0, forward_only: bool = False):
    """e = 0, any k: per length the k-mer byte strings of the text (and of its reverse complement) counted in a dict, looked up with the
    query's k-mers.  A window with a byte outside A/C/G/T equals no k-mer of A/C/G/T, so validity needs no rule of its own here."""
    run = run_lengths(qbuf)
    limit = np.minimum(run, max_k)
    out = np.where(limit < min_k, INVALID, 0).astype(np.uint32)
    todo = set(np.nonzero(limit >= min_k)[0].tolist())
    texts = [text] if forward_only else [text, text.translate(_RC)[::-1]]
    for k in range(min_k, max_k + 1):
        todo = {p for p in todo if limit[p] >= k}
        if not todo:
            break
        need = {qbuf[p:p + k] for p in todo}
        cnt = Counter()
        for tt in texts:
            cnt.update(w for w in (tt[q:q + k] for q in range(len(tt) - k + 1)) if w in need)
        done = {p for p in todo if cnt[qbuf[p:p + k]] <= t}
        for p in done:
            out[p] = k
        todo -= done
    return out


def split(vals, records):
    return Q.split(vals, records)


def bedgraph(vals_per_record, names) -> bytes:
    """the bytes `dicey mappability -q -l` writes: one line per maximal run of equal lengths; 0 (no length) and INVALID have no line"""
    out = []
    for name, v in zip(names, vals_per_record):
        v = np.asarray(v).astype(np.int64)
        if not len(v):
            continue
        starts = np.nonzero(np.concatenate([[True], v[1:] != v[:-1]]))[0]
        ends = np.concatenate([starts[1:], [len(v)]])
        for a, b in zip(starts.tolist(), ends.tolist()):
            if v[a] != INVALID and v[a] != 0:
                out.append(b"%s\t%d\t%d\t%d\n" % (name.encode(), a, b, v[a]))
    return b"".join(out)


def _clean(t, start, m):
    """the first position >= start from which m characters of t are all A/C/G/T"""
    return next(a for a in range(start, len(t) - m) if set(t[a:a + m]) <= set("ACGT"))


def _revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def record_set(seqs, text: bytes, min_k: int = 10, max_k: int = 24):
    """the query shapes at which the kernel can go wrong, at their smallest, for the three-sequence session genome (tests/conftest.py
    small_genome): list of bytes"""
    t = text.decode()
    s1, s2, s3 = seqs
    rng = random.Random(43)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    a = next(a for a in range(1000, 25000) if "N" in s1[a + 100:a + 2900] and set(s1[a:a + 40] + s1[a + 2960:a + 3000]) <= set("ACGT"))
    b, c = _clean(s2, 5000, 600), _clean(s3, 9000, 800)
    j0, j1 = _clean(s1, 20000, 60), _clean(s3, 2000, 60)
    x, z = _clean(s2, 12000, max_k), _clean(s3, 20000, 300)
    sub = list(s3[c:c + 800])
    for i in range(6, 800, 13):
        sub[i] = "ACGT"[("ACGT".index(sub[i]) + 1 + i % 3) % 4]
    recs = [s1[a:a + 3000],                                  # first record, buffer offset 0: a cut with an N run
            _revcomp(s2[b:b + 600]),                         # the other strand of a cut
            "".join(sub),                                    # one substitution every 13 nt
            s1[j0:j0 + 60] + s3[j1:j1 + 60],                 # a two-exon junction
            rnd(500),
            s2[x:x + min_k], s2[x:x + max_k], s2[x + 1:x + 13], s2[x + 2:x + 18],  # exactly min_k, max_k, and the (12, 16) pair
            rnd(9), "",                                      # shorter than every k, empty
            s1[j0:j0 + 100].lower()]                         # lower case: invalid (bytes go through as given)
    # the genome's own six longest repeated stretches (20-mers that occur twice or more), and a record that ends min_k + 3 nt behind one
    v20 = R.values(text, 20)
    starts, lens, _ = R.runs((v20 >= 2).astype(np.uint32), 0, len(text))
    order = np.argsort(-lens.astype(np.int64), kind="stable")[:6]
    for i in order:
        recs.append(t[int(starts[i]):int(starts[i]) + int(lens[i]) + 19])
    i = int(order[0])
    end = int(starts[i]) + int(lens[i]) + 19
    tail = t[end:end + min_k + 3]
    if set(tail) <= set("ACGT") and len(tail) == min_k + 3:
        recs.append(t[int(starts[i]):end] + tail)
    recs.append("A" * 40)                                    # a homopolymer
    recs.append(s3[z:z + 300])                               # last record: a cut whose final window is valid
    return [r.encode() for r in recs]
