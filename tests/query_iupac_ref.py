"""Brute-force degenerate query mappability, independent of the FM-index: the expected values of dg_query_map_iupac
(include/dicey_gpu.h).  The letters of a record are A, C, G, T and the IUPAC codes R Y S W K M B D H V N, each a set S(c) of bases, kept
as a 4-bit mask (A = 1, C = 2, G = 4, T = 8).  For a record Q, a position p, w = Q[p, p+k) of these 15 letters and an anchor a in 0..k:
  deg(w)     = the product of |S(w_j)|
  dist(u, w) = #{ j : u_j not in S(w_j) }
  fwd(p)     = #{valid windows u of the TEXT : dist(u, w) <= e and u_j in S(w_j) for the LAST a indices j}
  rev(p)     = the same against revcomp(w): the complemented sets in reverse order, anchored at the FIRST a indices
p is valid when such a w starts there and deg(w) <= max_degeneracy; text windows are A/C/G/T only.

`parts` is query_anchor_ref.parts_diagonal with sets: for every shift between the query buffer and the text, and between it and the
complemented reverse of the text, one inequality vector `(query set & text base bit) == 0`, a cumulative sum, window sums.  The
cumulative sum does not depend on k, so all k of a call share it.  The complemented set is the 4-bit mask reversed; deg is a log-sum over
the window.  Two deliberately wrong variants serve conditions on the inputs only: `first` replaces each code by its lowest member, `wild`
by N.  The `dbl` mask marks the positions that have a counted window with an out-of-set base at a degenerate index: a sum over the
expansions of w counts such a window more than once."""
import itertools
import random

import numpy as np

INVALID = 0xFFFFFFFF
SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
LETTER = {m: c for c, m in SETS.items()}
POP = np.array([bin(i).count("1") for i in range(16)], np.uint8)
COMP_MASK = np.array([int(format(i, "04b")[::-1], 2) for i in range(16)], np.uint8)  # A <-> T, C <-> G: the four bits reversed
_QSET = np.zeros(256, np.uint8)
for _c, _m in SETS.items():
    _QSET[ord(_c)] = _m
_TBIT = np.zeros(256, np.uint8)
for _c in "ACGT":
    _TBIT[ord(_c)] = SETS[_c]


def complement(c: str) -> str:
    return LETTER[int(COMP_MASK[SETS[c]])]


def revcomp(s: str) -> str:
    return "".join(complement(c) for c in reversed(s))


def deg(w: str) -> int:
    """the number of expansions of w; 0 when w holds a letter outside the 15"""
    n = 1
    for c in w:
        n *= int(POP[SETS.get(c, 0)])
    return n


def expansions(w: str):
    """every concrete expansion of w, the sets' members in A, C, G, T order"""
    return ["".join(t) for t in itertools.product(*[[b for b in "ACGT" if SETS[b] & SETS[c]] for c in w])]


def query_sets(qbuf: bytes, variant="right"):
    q = _QSET[np.frombuffer(qbuf, np.uint8)]
    if variant == "first":
        q = q & (~q + 1).astype(np.uint8)
    elif variant == "wild":
        q = np.where(POP[q] > 1, 15, q).astype(np.uint8)
    else:
        assert variant == "right"
    return q


def _window_all(ok, k):
    """bit p = ok holds at all of [p, p + k); as long as ok, False where the window runs past the end"""
    z = np.concatenate([[0], np.cumsum(~ok)])
    out = np.zeros(len(ok), bool)
    if len(ok) >= k:
        out[:len(ok) - k + 1] = (z[k:] - z[:-k]) == 0
    return out


def degeneracy(qbuf: bytes, k: int):
    """(letters, deg): letters[p] = a k-mer of the 15 letters starts at p; deg[p] = its number of expansions (0 where none starts)"""
    s = _QSET[np.frombuffer(qbuf, np.uint8)]
    letters = _window_all(s != 0, k)
    lg = np.concatenate([[0.0], np.cumsum(np.log2(np.maximum(POP[s], 1).astype(np.float64)))])  # (log2 of a uint8 array is float16)
    d = np.zeros(len(s), np.int64)
    if len(s) >= k:
        d[:len(s) - k + 1] = np.rint(2.0 ** (lg[k:] - lg[:-k])).astype(np.int64)  # products of 2s and 3s far below 2^53: exact
    d[~letters] = 0
    return letters, d


def parts(text: bytes, qbuf: bytes, ks, es, anchors, max_degeneracy=4096, variant="right"):
    """({(k, e, a): (fwd, rev, valid)}, {(k, e): dbl}) over the positions of the query buffer; anchors: {k: [a, ...]}; dbl at anchor 0"""
    t = _TBIT[np.frombuffer(text, np.uint8)]
    q = query_sets(qbuf, variant)
    isdeg = POP[_QSET[np.frombuffer(qbuf, np.uint8)]] > 1
    ks = sorted(ks)
    valid, vt = {}, {}
    for k in ks:
        letters, d = degeneracy(qbuf, k)
        valid[k] = letters & (d <= max_degeneracy)
        vt[k] = _window_all(t != 0, k)
    acc = {(k, e, a): (np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)) for k in ks for e in es for a in anchors[k]}
    dbl = {(k, e): np.zeros(len(q), bool) for k in ks for e in es}
    k0, emax = ks[0], max(es)
    nq0, nt0 = len(q) - k0 + 1, len(t) - k0 + 1
    for strand, tt in enumerate((t, COMP_MASK[t][::-1])):
        vts = {k: (vt[k] if strand == 0 else np.concatenate([vt[k][:len(t) - k + 1][::-1], np.zeros(k - 1, bool)])) for k in ks}
        for d in range(-(nq0 - 1), nt0):  # the query window at p against the text window at p + d
            p0, p1 = max(0, -d), min(nq0, nt0 - d)  # window starts at the smallest k
            if p1 <= p0:
                continue
            neq = (q[p0:p1 + k0 - 1] & tt[p0 + d:p1 + d + k0 - 1]) == 0
            cs = np.concatenate([[0], np.cumsum(neq, dtype=np.int32)])
            # a pair within e at a larger k holds a pair within e at the smallest one, at the same starts
            if not (valid[k0][p0:p1] & vts[k0][p0 + d:p1 + d] & (cs[k0:] - cs[:len(cs) - k0] <= emax)).any():
                continue
            cm = np.concatenate([[0], np.cumsum(neq & isdeg[p0:p1 + k0 - 1], dtype=np.int32)])
            for k in ks:
                n = len(cs) - k  # windows of this k on the stretch
                if n <= 0:
                    continue
                ham = cs[k:] - cs[:n]
                both = valid[k][p0:p0 + n] & vts[k][p0 + d:p0 + d + n]
                miss = cm[k:] - cm[:n]
                for a in anchors[k]:
                    tail = both & (cs[k:] - cs[k - a:k - a + n] == 0)  # the query window's last a indices
                    for e in es:
                        hit = tail & (ham <= e)
                        acc[k, e, a][strand][p0:p0 + n] += hit
                        if a == 0:
                            dbl[k, e][p0:p0 + n] |= hit & (miss > 0)
    return {key: (acc[key][0], acc[key][1], valid[key[0]]) for key in acc}, dbl


def _clean(t, start, m):
    return next(a for a in range(start, len(t) - m) if set(t[a:a + m]) <= set("ACGT"))


def put_codes(s, every, kind, rng):
    """s with a code every `every` letters: `miss` a two-letter code that excludes the base there, `hit` a two- or three-letter code that
    contains it, `N` an N"""
    s = list(s)
    for i in range(every // 2, len(s), every):
        b = SETS[s[i]]
        if kind == "miss":
            c = [x for x, m in SETS.items() if POP[m] == 2 and not (m & b)]
        elif kind == "hit":
            c = [x for x, m in SETS.items() if POP[m] in (2, 3) and (m & b)]
        else:
            c = ["N"]
        s[i] = rng.choice(c)
    return "".join(s)


TOO_DEGENERATE = "ACGTNNNNNNNACGTACGTACGTAC"  # seven N's: 16384 expansions where a window covers them all


def record_set(seqs):
    """the query shapes at which the degenerate kernel can go wrong, for the three-sequence session genome (tests/conftest.py
    small_genome); list of bytes"""
    s1, s2, s3 = seqs
    rng = random.Random(53)
    b, c, d, g, h = _clean(s2, 5000, 600), _clean(s3, 9000, 600), _clean(s1, 8000, 400), _clean(s2, 16000, 600), _clean(s3, 15000, 400)
    x12, x16, x20 = _clean(s2, 12000, 12), _clean(s2, 13000, 16), _clean(s2, 14000, 20)
    recs = [put_codes(s2[b:b + 600], 23, "miss", rng),          # first record, buffer offset 0: a miss code every 23 nt
            put_codes(s3[c:c + 600], 11, "hit", rng),           # a hit code every 11
            put_codes(s1[d:d + 400], 29, "N", rng),             # an N every 29
            revcomp(put_codes(s2[g:g + 600], 23, "miss", rng)),  # the other strand, the codes complemented
            revcomp(put_codes(s3[h:h + 400], 7, "hit", rng)),
            TOO_DEGENERATE,
            put_codes(s2[x12:x12 + 12], 12, "hit", rng), put_codes(s2[x16:x16 + 16], 16, "miss", rng), s2[x20:x20 + 20],  # records of exactly k
            "ACGTRYKMA", "",                                    # shorter than every k, empty
            put_codes(s1[d:d + 100], 11, "hit", rng).lower(),   # lower case: invalid (bytes go through as given)
            s3[c:c + 30] + "U" + s3[c + 31:c + 60],             # U is no letter here
            s1[d:d + 300]]                                      # last record: no code at all, its final window valid
    return [r.encode() for r in recs]


def finish(fwd, rev, valid, forward_only=False, max_count=0):
    """query_map_ref.finish: the saturated, capped totals with INVALID at invalid positions"""
    out = fwd.astype(np.uint64) + (0 if forward_only else rev.astype(np.uint64))
    out = np.minimum(out, INVALID - 1)
    if max_count:
        out = np.minimum(out, max_count)
    out[~valid] = INVALID
    return out.astype(np.uint32)


KS, ES = (12, 16, 20), (0, 1, 2)


def anchors_of(k):
    return [0, 1, 5, k]


_session = {}


def session(seqs, text):
    """the record set on the session genome and its `parts` at KS x ES x anchors_of(k), computed once per process"""
    key = hash(text)
    if key not in _session:
        recs = record_set(seqs)
        qbuf = b"".join(r + b"\n" for r in recs)
        p, dbl = parts(text, qbuf, KS, ES, {k: anchors_of(k) for k in KS})
        _session[key] = {"recs": recs, "qbuf": qbuf, "parts": p, "dbl": dbl}
    return _session[key]
