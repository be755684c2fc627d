"""Brute-force query mappability, independent of the FM-index: the expected values of dg_query_map (include/dicey_gpu.h).
For a record Q and a valid position p (p + k <= len(Q), Q[p, p+k) all A/C/G/T): value_e(p) = #{valid windows q of the TEXT :
Hamming(T[q, q+k), w) <= e} + the same against revcomp(w), w = Q[p, p+k); invalid positions carry INVALID; 0 is a value.

Two references that share nothing but the valid-position rule (mappability_ref.valid_positions):
  ball      k <= 32: the text's valid windows as 2-bit codes with their counts, looked up over the XOR-mask Hamming ball of the query
            k-mer's code and of its reverse complement's;
  diagonal  any k: for every shift between the query buffer and the text, and between it and revcomp(text), one inequality vector, a
            cumulative sum, window sums, valid pairs within e counted.  Cost (|Q| + |T|) * |Q|.
`ball_at` counts a handful of positions of a text too large for either, `bedgraph` writes what `dicey mappability -q` writes."""
import numpy as np

import mappability_mm_ref as M
import mappability_ref as R

INVALID = 0xFFFFFFFF
SATURATED = 0xFFFFFFFE


def buffer_of(records):
    """the records laid out like an index text: REC1 '\\n' REC2 '\\n' ... ; and the offset of each record in it"""
    offs, o = [], 0
    for r in records:
        offs.append(o)
        o += len(r) + 1
    return b"".join(r + b"\n" for r in records), offs


def _codes(buf: bytes, pos, k):
    """(code of the k-mer at each pos, code of its reverse complement), first character most significant"""
    c = R._CODE[np.frombuffer(buf, dtype=np.uint8)].astype(np.uint64)
    c[c == 255] = 0
    fw = np.zeros(len(pos), dtype=np.uint64)
    rc = np.zeros(len(pos), dtype=np.uint64)
    for j in range(k):
        cj = c[pos + j]
        fw = (fw << np.uint64(2)) | cj
        rc |= (np.uint64(3) - cj) << np.uint64(2 * j)
    return fw, rc


def _text_table(text: bytes, k: int):
    pos = np.nonzero(R.valid_positions(text, k))[0]
    if not len(pos):
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    keys, cnt = np.unique(_codes(text, pos, k)[0], return_counts=True)
    return keys, cnt.astype(np.int64)


def _look(keys, cnt, q):
    if not len(keys):
        return np.zeros(len(q), dtype=np.int64)
    ix = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return np.where(keys[ix] == q, cnt[ix], 0)


def parts_ball(text: bytes, qbuf: bytes, k: int, e: int):
    """(fwd_e, rev_e, valid) over the positions of the query buffer; k <= 32"""
    assert k <= 32
    valid = R.valid_positions(qbuf, k)
    fwd = np.zeros(len(qbuf), dtype=np.int64)
    rev = np.zeros(len(qbuf), dtype=np.int64)
    pos = np.nonzero(valid)[0]
    if len(pos):
        keys, cnt = _text_table(text, k)
        fw, rc = _codes(qbuf, pos, k)
        ufw, ifw = np.unique(fw, return_inverse=True)
        urc, irc = np.unique(rc, return_inverse=True)
        sf = np.zeros(len(ufw), dtype=np.int64)
        sr = np.zeros(len(urc), dtype=np.int64)
        for m in M._masks(k, e):
            sf += _look(keys, cnt, ufw ^ m)
            sr += _look(keys, cnt, urc ^ m)
        fwd[pos] = sf[ifw]
        rev[pos] = sr[irc]
    return fwd, rev, valid


def parts_diagonal(text: bytes, qbuf: bytes, k: int, es=(0, 1, 2)):
    """{e: (fwd_e, rev_e, valid)} over the positions of the query buffer"""
    t = np.frombuffer(text, dtype=np.uint8)
    q = np.frombuffer(qbuf, dtype=np.uint8)
    vq = R.valid_positions(qbuf, k)
    nq, nt = len(q) - k + 1, len(t) - k + 1  # window starts
    acc = {e: (np.zeros(len(q), dtype=np.int64), np.zeros(len(q), dtype=np.int64)) for e in es}
    if nq > 0 and nt > 0:
        vt = R.valid_positions(text, k)[:nt]
        # the window at r of rc = revcomp(T) is the reverse complement of T's window at nt-1-r, and Hamming(w, revcomp(u)) =
        # Hamming(revcomp(w), u)
        for strand, (tt, vv) in enumerate(((t, vt), (M._COMP[t][::-1], vt[::-1]))):
            for d in range(-(nq - 1), nt):  # the query window at p against the window at p + d
                p0, p1 = max(0, -d), min(nq, nt - d)
                if p1 <= p0:
                    continue
                neq = q[p0:p1 + k - 1] != tt[p0 + d:p1 + d + k - 1]
                cs = np.concatenate([[0], np.cumsum(neq, dtype=np.int32)])
                ham = cs[k:] - cs[:len(cs) - k]
                both = vq[p0:p1] & vv[p0 + d:p1 + d]
                for e in es:
                    acc[e][strand][p0:p1] += both & (ham <= e)
    return {e: (acc[e][0], acc[e][1], vq) for e in es}


def finish(fwd, rev, valid, forward_only=False, max_count=0):
    out = fwd.astype(np.uint64) + (0 if forward_only else rev.astype(np.uint64))
    out = np.minimum(out, SATURATED)
    if max_count:
        out = np.minimum(out, max_count)
    out[~valid] = INVALID
    return out.astype(np.uint32)


def split(vals, records):
    """the buffer's values record by record (the '\\n' positions dropped)"""
    _, offs = buffer_of(records)
    return [vals[o:o + len(r)] for o, r in zip(offs, records)]


def values(text: bytes, records, k: int, e: int, forward_only=False, max_count=0, method="ball"):
    """list of uint32 arrays, one per record"""
    qbuf, _ = buffer_of(records)
    parts = parts_ball(text, qbuf, k, e) if method == "ball" else parts_diagonal(text, qbuf, k, (e,))[e]
    return split(finish(*parts, forward_only, max_count), records)


def ball_at(text: bytes, kmers, k: int, e: int, forward_only=False):
    """value_e of a few k-mers (bytes of A/C/G/T), each by summing the text's window counts over its explicit Hamming ball; k <= 32"""
    keys, cnt = _text_table(text, k)
    masks = M._masks(k, e)
    out = []
    for w in kmers:
        fw, rc = _codes(w, np.array([0]), k)
        n = int(_look(keys, cnt, fw[0] ^ masks).sum())
        if not forward_only:
            n += int(_look(keys, cnt, rc[0] ^ masks).sum())
        out.append(n)
    return np.array(out, dtype=np.int64)


def bedgraph(vals_per_record, names) -> bytes:
    """the bytes `dicey mappability -q` writes: one line per maximal run of equal values over valid positions, zero included"""
    out = []
    for name, v in zip(names, vals_per_record):
        v = np.asarray(v).astype(np.int64)
        if not len(v):
            continue
        starts = np.nonzero(np.concatenate([[True], v[1:] != v[:-1]]))[0]
        ends = np.concatenate([starts[1:], [len(v)]])
        for a, b in zip(starts.tolist(), ends.tolist()):
            if v[a] != INVALID:
                out.append(b"%s\t%d\t%d\t%d\n" % (name.encode(), a, b, v[a]))
    return b"".join(out)
