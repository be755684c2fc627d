"""Brute-force k-mer counts over a text, independent of the FM-index: the expected values of dg_mappability
(include/dicey_gpu.h) and the bedGraph `dicey mappability` writes."""
from collections import Counter

import numpy as np

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def valid_positions(text: bytes, k: int) -> np.ndarray:
    """bool[len(text)]: the k bytes from p lie inside the text and are all A/C/G/T"""
    t = np.frombuffer(text, dtype=np.uint8)
    L = len(t)
    bad = _CODE[t] == 255
    cs = np.concatenate([[0], np.cumsum(bad, dtype=np.int64)])
    v = np.zeros(L, dtype=bool)
    if k <= L:
        v[:L - k + 1] = (cs[k:] - cs[:L - k + 1]) == 0
    return v


def values(text: bytes, k: int, forward_only: bool = False, max_count: int = 0) -> np.ndarray:
    """uint32[len(text)] = value of every position (the text's length is the index's n - 1)"""
    L = len(text)
    v = valid_positions(text, k)
    out = np.zeros(L, dtype=np.uint64)
    pos = np.nonzero(v)[0]
    if len(pos):
        if k <= 32:
            c = _CODE[np.frombuffer(text, dtype=np.uint8)].astype(np.uint64)
            c[c == 255] = 0
            fw = np.zeros(len(pos), dtype=np.uint64)
            rc = np.zeros(len(pos), dtype=np.uint64)
            for j in range(k):
                cj = c[pos + j]
                fw = (fw << np.uint64(2)) | cj
                rc |= (np.uint64(3) - cj) << np.uint64(2 * j)
            keys, cnt = np.unique(fw, return_counts=True)
            val = cnt[np.searchsorted(keys, fw)].astype(np.uint64)
            if not forward_only:
                ix = np.minimum(np.searchsorted(keys, rc), len(keys) - 1)
                val += np.where(keys[ix] == rc, cnt[ix], 0).astype(np.uint64)
        else:
            comp = bytes.maketrans(b"ACGT", b"TGCA")
            ws = [text[p:p + k] for p in pos.tolist()]
            cnt = Counter(ws)
            val = np.array([cnt[w] + (0 if forward_only else cnt.get(w.translate(comp)[::-1], 0)) for w in ws], dtype=np.uint64)
        out[pos] = val
    out = np.minimum(out, 0xFFFFFFFF)
    if max_count:
        out = np.minimum(out, max_count)
    return out.astype(np.uint32)


def runs(vals: np.ndarray, lo: int, hi: int):
    """maximal runs of equal non-zero values inside [lo, hi): (start, length, value) arrays"""
    v = vals[lo:hi].astype(np.int64)
    if len(v) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    change = np.concatenate([[True], v[1:] != v[:-1]])
    starts = np.nonzero(change)[0]
    ends = np.concatenate([starts[1:], [len(v)]])
    keep = v[starts] != 0
    s, e = starts[keep], ends[keep]
    return (s + lo).astype(np.uint64), (e - s).astype(np.uint32), v[s].astype(np.uint32)


def bedgraph(text: bytes, names, k: int, forward_only: bool = False, max_count: int = 0) -> bytes:
    """the bytes `dicey mappability` writes for the genome whose index text is `text` (sequences in FASTA order)"""
    vals = values(text, k, forward_only, max_count)
    out = []
    off = 0
    for name, seq in zip(names, text.split(b"\n")[:-1]):
        s, ln, v = runs(vals, off, off + len(seq))
        for a, b, c in zip((s - off).tolist(), ln.tolist(), v.tolist()):
            out.append(b"%s\t%d\t%d\t%d\n" % (name.encode(), a, a + b, c))
        off += len(seq) + 1
    return b"".join(out)
