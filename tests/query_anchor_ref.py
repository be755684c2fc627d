"""Brute-force anchored query mappability, independent of the FM-index: the expected values of dg_query_map_anchored
(include/dicey_gpu.h).  For a record Q, a valid position p, w = Q[p, p+k) and an anchor a in 0..k:
  fwd(p) = #{valid windows u of the TEXT : Hamming(u, w) <= e and u[k-a, k) == w[k-a, k)}
  rev(p) = #{valid windows u of the TEXT : Hamming(u, revcomp(w)) <= e and u[0, a) == revcomp(w)[0, a)}
The anchored bases are always the LAST a bases of the oligo w; on the other strand the text shows them as the first a of the window.

Two references beside those of query_map_ref, sharing its valid-position rule and nothing else with each other:
  ball      k <= 32: the XOR masks of the Hamming ball (mappability_mm_ref._masks; codes carry the first character in the most significant
            bits).  The forward strand keeps the masks with no bit in the low 2a bits, the reverse strand (the code of revcomp(w)) those
            with no bit from 2(k-a) up.  Every mask is looked up once and added to every anchor it satisfies, so all anchors of a (k, e)
            cost one unanchored pass;
  diagonal  any k: query_map_ref.parts_diagonal's shifts with the extra condition that the last a positions of the QUERY window hold no
            inequality, on both strands (the text is what is reverse-complemented there)."""
import random

import numpy as np

import mappability_mm_ref as M
import mappability_ref as R
import query_map_ref as Q


def parts_ball(text: bytes, qbuf: bytes, k: int, e: int, anchors):
    """{a: (fwd, rev, valid)} over the positions of the query buffer; k <= 32"""
    assert k <= 32 and all(0 <= a <= k for a in anchors)
    valid = R.valid_positions(qbuf, k)
    out = {a: (np.zeros(len(qbuf), dtype=np.int64), np.zeros(len(qbuf), dtype=np.int64), valid) for a in anchors}
    pos = np.nonzero(valid)[0]
    if not len(pos):
        return out
    keys, cnt = Q._text_table(text, k)
    fw, rc = Q._codes(qbuf, pos, k)
    ufw, ifw = np.unique(fw, return_inverse=True)
    urc, irc = np.unique(rc, return_inverse=True)
    sf = {a: np.zeros(len(ufw), dtype=np.int64) for a in anchors}
    sr = {a: np.zeros(len(urc), dtype=np.int64) for a in anchors}
    for m in M._masks(k, e):
        mi = int(m)
        lf = Q._look(keys, cnt, ufw ^ m)
        lr = Q._look(keys, cnt, urc ^ m)
        # character index j of the window sits at bits 2(k-1-j): the last a characters are the low 2a bits, the first a those from 2(k-a) up
        low = ((mi & -mi).bit_length() - 1) // 2 if mi else k   # characters behind the LAST substituted one
        high = (mi.bit_length() - 1) // 2 if mi else -1         # k-1-high characters in front of the FIRST substituted one
        for a in anchors:
            if a <= low:
                sf[a] += lf
            if a <= k - 1 - high:
                sr[a] += lr
    for a in anchors:
        out[a][0][pos] = sf[a][ifw]
        out[a][1][pos] = sr[a][irc]
    return out


def parts_diagonal(text: bytes, qbuf: bytes, k: int, es, anchors):
    """{(e, a): (fwd, rev, valid)} over the positions of the query buffer"""
    t = np.frombuffer(text, dtype=np.uint8)
    q = np.frombuffer(qbuf, dtype=np.uint8)
    vq = R.valid_positions(qbuf, k)
    nq, nt = len(q) - k + 1, len(t) - k + 1
    acc = {(e, a): (np.zeros(len(q), dtype=np.int64), np.zeros(len(q), dtype=np.int64)) for e in es for a in anchors}
    if nq > 0 and nt > 0:
        vt = R.valid_positions(text, k)[:nt]
        for strand, (tt, vv) in enumerate(((t, vt), (M._COMP[t][::-1], vt[::-1]))):
            for d in range(-(nq - 1), nt):  # the query window at p against the window at p + d
                p0, p1 = max(0, -d), min(nq, nt - d)
                if p1 <= p0:
                    continue
                neq = q[p0:p1 + k - 1] != tt[p0 + d:p1 + d + k - 1]
                cs = np.concatenate([[0], np.cumsum(neq, dtype=np.int32)])
                n = len(cs) - k  # windows
                ham = cs[k:] - cs[:n]
                both = vq[p0:p1] & vv[p0 + d:p1 + d]
                for a in anchors:
                    tail = both & (cs[k:] - cs[k - a:k - a + n] == 0)  # the query window's last a positions
                    for e in es:
                        acc[e, a][strand][p0:p1] += tail & (ham <= e)
    return {key: (acc[key][0], acc[key][1], vq) for key in acc}


def table_reads(k: int, e: int, a: int, K: int, forward_only: bool) -> int:
    """K-mer table entries one valid position reads (no max_count): per strand 1 + 3F + 9F(F-1)/2 with F free steps among the table's K"""
    if not K or k < K:
        return 0
    per = lambda F: 1 + (3 * F if e >= 1 else 0) + (9 * F * (F - 1) // 2 if e >= 2 else 0)
    return per(K - min(a, K)) + (0 if forward_only else per(min(K, k - a)))


def _clean(t, start, m):
    return next(a for a in range(start, len(t) - m) if set(t[a:a + m]) <= set("ACGT"))


def _revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _subst_every(s, every):
    s = list(s)
    for i in range(every // 2, len(s), every):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + i % 3) % 4]
    return "".join(s)


def record_set(seqs):
    """the query shapes at which the anchored kernel can go wrong, for the three-sequence session genome (tests/conftest.py small_genome):
    cuts of both strands with substitutions every 23 and every 11 nt, so that single- and double-substitution windows carry a
    substitution inside and outside every anchor used; list of bytes"""
    s1, s2, s3 = seqs
    rng = random.Random(47)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    a = next(a for a in range(1000, 25000) if "N" in s1[a + 100:a + 2900] and set(s1[a:a + 40] + s1[a + 2960:a + 3000]) <= set("ACGT"))
    b, c, d = _clean(s2, 5000, 600), _clean(s3, 9000, 800), _clean(s1, 8000, 400)
    g, h = _clean(s2, 16000, 600), _clean(s3, 15000, 400)
    j0, j1 = _clean(s1, 20000, 60), _clean(s3, 2000, 60)
    x12, x16, x20, z = _clean(s2, 12000, 12), _clean(s2, 13000, 16), _clean(s2, 14000, 20), _clean(s3, 20000, 300)
    recs = [s1[a:a + 3000],                                  # first record, buffer offset 0: a cut with an N run
            _revcomp(s2[b:b + 600]),                         # the other strand of a cut
            _subst_every(s3[c:c + 800], 23),                 # one substitution every 23 nt
            _subst_every(s1[d:d + 400], 11),                 # and every 11: two inside most windows
            _revcomp(_subst_every(s2[g:g + 600], 23)),       # the same on the other strand
            _revcomp(_subst_every(s3[h:h + 400], 11)),
            s1[j0:j0 + 60] + s3[j1:j1 + 60],                 # a two-exon junction
            rnd(500),
            s2[x12:x12 + 12], s2[x16:x16 + 16], s2[x20:x20 + 20],  # records of exactly k
            rnd(9), "",                                      # shorter than every k, empty
            s1[j0:j0 + 100].lower(),                         # lower case: invalid (bytes go through as given)
            s3[z:z + 300]]                                   # last record: a cut whose final window is valid
    return [r.encode() for r in recs]
