"""tests/index_layout_ref.py, the model of the layouts an index open derives, held against brute force on small texts — and every
comparer of it shown to accept a numpy emulation of what the kernels store and to reject the faults that leave every query result
intact: one spurious filter bit, an escape bit forced on, a wide flag at width 65535, block-minima padding of 0, a prefix-level flag
for the position that equals the level's X.  Also the preconditions of the four texts tests/test_gpu_index_layout.py opens.  No GPU."""
import random

import numpy as np
import pytest

import index_layout_ref as R
from conftest import genome_text, make_genome

U32, U64 = np.uint32, np.uint64


def small_texts():
    rng = random.Random(5)
    out = [b"A\n", b"ACGT\n", b"AAAAAAAAAAAAAAAAAAAAAAAAA\n", b"ACACACACACACACACACACACACAC\nACACACACA\n", b"NNNNACGTNACGTRACGTN\nAC\n"]
    for _ in range(6):
        seqs = make_genome(rng.randrange(1000), 2, rng.randint(100, 300), nrate=0.02, iupac=True)
        out.append(genome_text(seqs))
    return out


SMALL = small_texts()


@pytest.fixture(scope="module")
def tiny():
    """one text of a few thousand symbols with N runs, repeats, IUPAC letters and a short last sequence: the comparers' subject"""
    seqs = make_genome(77, 2, 1500, nrate=0.01, iupac=True) + ["ACG"]
    return R.Model(genome_text(seqs))


@pytest.fixture(scope="module")
def models():
    return {name: R.Model(R.text_of(name)[0]) for name in R.TEXT_NAMES}


def count_overlapping(text, pat):
    c, i = 0, text.find(pat)
    while i >= 0:
        c, i = c + 1, text.find(pat, i + 1)
    return c


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_suffix_array_is_the_sorted_suffixes(k):
    full = SMALL[k] + b"\0"
    want = sorted(range(len(full)), key=lambda p: full[p:])  # bytes compare unsigned; a proper prefix sorts first, the sentinel is 0
    assert R.suffix_array(full).tolist() == want


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_table_widths_are_overlapping_counts(k):
    m = R.Model(SMALL[k])
    for K in (1, 2, 3, 5):
        lo, width, wide, pre = m.ktab(K)
        for code in range(4 ** K):
            pat = bytes(b"ACGT"[(code >> (2 * (K - 1 - j))) & 3] for j in range(K))  # first character on top
            assert width[code] == count_overlapping(m.text, pat), (K, pat)
            if width[code]:
                assert all(m.full[p:p + K] == pat for p in m.sa[lo[code]:lo[code] + width[code]])
                assert pre[code] == m.pre5()[lo[code]] & 0x7FFF
            else:
                assert lo[code] == 0 and pre[code] == 0x7FFF
        assert not wide.any()


def test_model_pieces_against_loops(tiny):
    """Occ, C4, the N runs, pre5, the sax context and the block minima once more, as loops over the text"""
    m, n, full, sa = tiny, tiny.n, tiny.full, tiny.sa
    bwt = [full[p - 1] if p else 0 for p in sa]
    code_of = lambda b: {65: 0, 67: 1, 71: 2, 84: 3, 78: 4, 10: 5, 0: 6}.get(b, 7)  # noqa: E731
    cnt, planes, mask = m.occ()
    assert len(cnt) == (n >> 7) + 1
    for b in range(len(cnt)):
        assert cnt[b].tolist() == [sum(code_of(x) == c for x in bwt[:128 * b]) for c in range(4)]
        for w in range(2):
            for pl in range(3):
                want = sum(((code_of(bwt[i]) >> pl) & 1) << (i - 128 * b - 64 * w) for i in range(128 * b + 64 * w, min(n, 128 * b + 64 * w + 64)))
                assert int(planes[b, pl, w]) == want
            assert int(mask[b, w]) == sum(1 << j for j in range(64) if 128 * b + 64 * w + j < n)
    assert m.C4() == [sum(x < c for x in full) for c in b"ACGT"]
    import re
    runs = [len(r) for r in re.findall(rb"N+", m.text)]
    assert m.nrun_min() == min(64, min(runs))
    c3 = lambda p: (b"ACGT".index(full[p]) if 0 <= p < n and full[p] in b"ACGT" else 7)  # noqa: E731
    pos, esc, ctx = m.sax()
    for i in range(n):
        p = int(sa[i])
        assert m.pre5()[i] == sum(c3(p - k) << (3 * (k - 1)) for k in range(1, 6))
        window = [c3(p - 1), c3(p - 2)] + [c3(p + 16 + j) for j in range(13)]
        assert pos[i] == p and bool(esc[i]) == any(c > 3 for c in window)
        if not esc[i]:
            assert int(ctx[i]) == sum(c << (2 * j) for j, c in enumerate(window))
    prev = [int(v) for v in sa]
    for lv in m.samin():
        nout = (len(prev) + 7) // 8
        assert len(lv) == ((nout + 7) & ~7) + 8 and lv[:nout].tolist() == [min(prev[8 * b:8 * b + 8]) for b in range(nout)]
        assert (lv[nout:] == 0xFFFFFFFF).all()
        prev = lv[:nout].tolist()
    assert len(prev) <= 8


@pytest.mark.parametrize("k", [9, 10, 11, 12, 13, 14])
def test_filter_addressing_is_a_bijection(k):
    """every (k, s) the layouts can use: the fields kf_layout spreads over a 2k-bit code, and the edges 0 and 2k - 9"""
    bits = 2 * k
    nr = min(4, (bits - 9 + 7) // 8 + 1)
    ss = {(r * (bits - 9) + (nr - 1) // 2) // (nr - 1) for r in range(nr)} | {0, bits - 9}
    codes = np.arange(1 << bits, dtype=np.uint64) if bits <= 24 else None
    for s in sorted(ss):
        if codes is not None:
            addr = R.filter_address(codes, k, s)
            seen = np.zeros(1 << bits, bool)
            seen[addr] = True  # (an address past the range raises)
            assert seen.all(), (k, s)  # onto a set of its own size: one to one
            assert np.array_equal(R.filter_code_of_address(addr, k, s), codes)
            some = np.unique(codes[:: 4097][:3000])
            marks = np.zeros(1 << bits, np.uint8)
            marks[addr[some.astype(np.int64)]] = 1
            assert np.array_equal(R.filter_yes_codes(np.packbits(marks, bitorder="little").view("<u4"), k, s), some)
        else:  # a field permutation: distinct on a random sample together with all its single-bit neighbours, and onto the range
            rng = np.random.default_rng(k * 100 + s)
            base = rng.integers(0, 1 << bits, 2000, dtype=np.uint64)
            sample = np.unique(np.concatenate([base] + [base ^ np.uint64(1 << b) for b in range(bits)]))
            addr = R.filter_address(sample, k, s)
            assert len(np.unique(addr)) == len(sample) and addr.max() < (1 << bits), (k, s)
            assert np.array_equal(R.filter_code_of_address(addr, k, s), sample)
            for b in range(bits):  # bit b of the code moves to exactly one bit of the address
                a = int(R.filter_address(np.array([1 << b], np.uint64), k, s)[0])
                assert bin(a).count("1") == 1


def test_the_layouts_fields_are_among_the_tested(models):
    """(k, s) of the default orders and of K = 12 / K2 = 14 on the four texts fall inside test_filter_addressing_is_a_bijection's range"""
    ks = {12, 14}
    for m in models.values():
        K, K2 = R.default_orders(m.n)
        ks |= {K, K2}
    assert {k for k in ks if 2 * k >= 17} <= {9, 10, 11, 12, 13, 14}


def test_text_preconditions(models):
    n = {k: m.n for k, m in models.items()}
    assert n["n40k"] <= 1 << 16 and (1 << 17) < n["n180k"] < (1 << 18) < n["n300k"]
    assert [len(R.plv_sizes(n[k])) for k in ("n40k", "n180k", "n300k", "wide")] == [0, 1, 2, 1]
    assert [R.default_orders(n[k]) for k in ("n40k", "n180k", "n300k", "wide")] == [(8, 10), (9, 11), (10, 12), (9, 11)]
    w = models["wide"]
    assert 135000 < w.n < 145000
    text, seqs = R.text_of("wide")
    import re
    for run in re.findall(r"A+|C+|G+|T+", "\n".join(seqs)):
        assert len(run) <= 5 or len(run) in (R.WIDE_A_RUN, R.WIDE_C_RUN)
    assert sorted(len(r) for r in re.findall(rb"N+", text)) == [1, 2, 63, 64, 65]
    assert sum(c not in b"ACGTN\n" for c in text) == 1 and min(len(s) for s in seqs) < 8 and text[-2] in b"ACGT" and text[-1:] == b"\n"
    lo, width, wide, pre = w.ktab(9)
    a9, c9 = 0, int("1" * 9, 4)
    assert width[a9] == 65536 and wide[a9] and width[c9] == 65535 and not wide[c9] and wide.sum() == 1
    assert width[a9] == count_overlapping(text, b"A" * 9) and width[c9] == count_overlapping(text, b"C" * 9)
    assert w.nrun_min() == 1
    for name, m in models.items():
        pos, esc, ctx = m.sax()
        print("%s: n %d, %d of the sax records escaped" % (name, m.n, esc.sum()))
        assert 2 * (~esc).sum() >= m.n, name
        if name != "wide":  # make_genome's N runs reach 150: the cap of 64 is not what these texts measure
            assert 1 <= m.nrun_min() <= 64


# ---- every comparer accepts the emulated kernels' output and rejects one flipped value ----

def rejects(fn, *a, match):
    with pytest.raises(AssertionError, match=match):
        fn(*a)


def occ_raw(m):
    cnt, planes, mask = m.occ()
    c = cnt.astype(U64)
    return np.concatenate(((c[:, 0] | (c[:, 1] << U64(32)))[:, None], (c[:, 2] | (c[:, 3] << U64(32)))[:, None], planes.reshape(len(cnt), 6)), axis=1)


def test_occ_comparer(tiny):
    raw = occ_raw(tiny)
    R.compare_occ(tiny, raw)
    junk = raw.copy()
    junk[-1, 2:] |= ~np.repeat(tiny.occ()[2][-1][None, :], 3, axis=0).reshape(-1)  # the tail of the last block is free
    R.compare_occ(tiny, junk)
    bad = raw.copy()
    bad[3, 1] += U64(1) << U64(32)
    rejects(R.compare_occ, tiny, bad, match=r"occ counts: first difference at index 3")
    bad = raw.copy()
    bad[2, 5] ^= U64(1) << U64(17)
    rejects(R.compare_occ, tiny, bad, match=r"occ planes: first difference at index 2")


@pytest.mark.parametrize("with_pre5", [True, False])
def test_ktab_comparer(models, with_pre5):
    w = models["wide"]
    lo, width, wide, pre = w.ktab(9, with_pre5)
    raw = R.pack_ktab(lo, width, np.where(wide, 0, pre))
    assert raw[0, 1] == 0x80010000 and raw[int("1" * 9, 4), 1] & 0xFFFF == 0xFFFF and not raw[int("1" * 9, 4), 1] >> 31
    R.compare_ktab(w, 9, raw, with_pre5)
    c9 = int("1" * 9, 4)
    bad = raw.copy()
    bad[c9, 1] = 0x80000000 | 65535  # the wide format one entry too early: decodes to the same interval
    rejects(R.compare_ktab, w, 9, bad, with_pre5, match=r"ktab wide flag: first difference at index %d" % c9)
    bad = raw.copy()
    bad[0, 1] = 0  # a wide entry whose width was cut to 16 bits
    rejects(R.compare_ktab, w, 9, bad, with_pre5, match=r"ktab width: first difference at index 0")
    bad = raw.copy()
    k = int(np.flatnonzero(width == 3)[0])
    bad[k, 1] ^= 1 << 20  # a preceding character of a narrow entry
    rejects(R.compare_ktab, w, 9, bad, with_pre5, match=r"ktab pre_first: first difference at index %d" % k)
    bad = raw.copy()
    k = int(np.flatnonzero(width == 0)[5])
    bad[k, 0] = 7
    rejects(R.compare_ktab, w, 9, bad, with_pre5, match=r"ktab lo: first difference at index %d" % k)
    if with_pre5:  # a table packed without pre5 is not the table of a handle that has it
        rejects(R.compare_ktab, w, 9, R.pack_ktab(lo, width, np.full(len(lo), 0x7FFF)), True, match=r"ktab pre_first")


def test_filter_comparer(tiny):
    k, s, pick = 9, [0, 5, 9, 0], 0
    for t in range(32):
        pick |= (t % 3) << (2 * t)
    copies = [tiny.filter_copy(k, s[r]).copy() for r in range(3)]
    R.compare_filter(tiny, "kf", k, 3, s, pick, copies)
    absent = int(np.setdiff1d(np.arange(1 << 18, dtype=np.uint64), tiny.present_codes(k))[1000])
    for r in range(3):  # one spurious bit in one copy: a false positive, every result stays right
        bad = [c.copy() for c in copies]
        a = int(R.filter_address(np.array([absent], np.uint64), k, s[r])[0])
        bad[r][a >> 5] |= U32(1 << (a & 31))
        rejects(R.compare_filter, tiny, "kf", k, 3, s, pick, bad, match=r"kf copy %d: \d+ bits set" % r)
    bad = [c.copy() for c in copies]  # the same number of bits, one of them moved
    a = int(R.filter_address(np.array([absent], np.uint64), k, s[1])[0])
    b = int(R.filter_address(tiny.present_codes(k)[:1], k, s[1])[0])
    bad[1][a >> 5] |= U32(1 << (a & 31))
    bad[1][b >> 5] &= ~U32(1 << (b & 31))
    rejects(R.compare_filter, tiny, "kf", k, 3, s, pick, bad, match=r"kf copy 1 \(s = 5\) words: first difference at index %d" % min(a >> 5, b >> 5))
    rejects(R.compare_filter, tiny, "kf", k, 3, s, pick | (3 << 10), copies, match=r"pick names copy 3 at window position 5")
    rejects(R.compare_filter, tiny, "kf", k, 3, [0, 5, 10, 0], pick, copies, match=r"in-line bits \[10, 19\)")


def test_sax_and_pre5_comparers(tiny):
    pos, esc, ctx = tiny.sax()
    raw = R.pack_sax(pos, esc, ctx)
    R.compare_sax(tiny, raw)
    R.compare_pre5(tiny, tiny.pre5().copy())
    junk = raw.copy()
    junk[esc, 1] ^= U32(0x2AAAAAAA)  # an escaped record's low bits are free
    R.compare_sax(tiny, junk)
    bad = raw.copy()
    bad[:, 1] |= U32(R.SAX_ESCAPE)  # escape always set: every hit reads the text again, the same hits come out
    first = int(np.flatnonzero(~esc)[0])
    rejects(R.compare_sax, tiny, bad, match=r"sax escape bit: first difference at index %d" % first)
    i = int(np.flatnonzero(~esc)[7])
    for bit in (0, 3, 4, 29, 30):
        bad = raw.copy()
        bad[i, 1] ^= U32(1 << bit)
        rejects(R.compare_sax, tiny, bad, match=r"sax context: first difference at index %d" % i)
    bad = raw.copy()
    bad[i, 0] += 1
    rejects(R.compare_sax, tiny, bad, match=r"sax position: first difference at index %d" % i)
    bad = tiny.pre5().copy()
    bad[11] ^= 1 << 14
    rejects(R.compare_pre5, tiny, bad, match=r"pre5: first difference at index 11")


def test_plv_comparer(tiny):
    x = 1024  # (the layouts start at 2^16; the format does not depend on it)
    sa = tiny.sa
    dir_raw = R.pack_plv_dir(sa, tiny.n, x)
    want_dir, idx = tiny.plv(x)
    assert len(idx) == x and (sa[idx] < x).all()
    sax_raw = R.pack_sax(*tiny.sax())
    rec = sax_raw[idx]
    R.compare_plv(tiny, 0, x, dir_raw, rec, sax_raw)
    # `<=` for `<`: the suffix at position x is flagged as well — one more record, one count off behind it
    dir_le = R.pack_plv_dir(sa, tiny.n, x + 1)
    i = int(np.flatnonzero(sa == x)[0])
    rejects(R.compare_plv, tiny, 0, x, dir_le, rec, match=r"plv\[0\] dir \(x = 1024\): first difference at index %d" % (i // R.PLV_LINE))
    rejects(R.compare_plv, tiny, 0, x, dir_raw, sax_raw[np.flatnonzero(sa <= x)], match=r"plv\[0\] rec: 1025 records")
    bad = dir_raw.copy()  # a flag at an index >= n
    bad[-1, 7] |= U64(1) << U64(63)
    assert (tiny.n // R.PLV_LINE) * R.PLV_LINE + 447 >= tiny.n
    rejects(R.compare_plv, tiny, 0, x, bad, rec, match=r"plv\[0\] dir .*index %d" % (len(bad) - 1))
    bad = rec.copy()
    bad[[5, 6]] = bad[[6, 5]]  # the records out of suffix-array order
    rejects(R.compare_plv, tiny, 0, x, dir_raw, bad, match=r"plv\[0\] rec position: first difference at index 5")
    bad = rec.copy()
    e = int(np.flatnonzero(tiny.sax()[1][idx])[0])
    bad[e, 1] ^= 1  # an escaped record must still be the sax entry itself
    R.compare_plv(tiny, 0, x, dir_raw, bad)
    rejects(R.compare_plv, tiny, 0, x, dir_raw, bad, sax_raw, match=r"plv\[0\] rec against sax: first difference at index %d" % e)


def test_samin_comparer(tiny):
    levels = [lv.copy() for lv in tiny.samin()]
    assert len(levels) >= 2
    R.compare_samin(tiny, levels)
    for j, lv in enumerate(levels):
        nout = int(np.flatnonzero(lv == 0xFFFFFFFF)[0])
        for at in (nout, len(lv) - 1):  # padding of 0 looks like a block whose minimum is position 0
            bad = [v.copy() for v in levels]
            bad[j][at] = 0
            rejects(R.compare_samin, tiny, bad, match=r"samin\[%d\]: first difference at index %d" % (j + 1, at))
    bad = [v.copy() for v in levels]
    bad[0][3] += 1
    rejects(R.compare_samin, tiny, bad, match=r"samin\[1\]: first difference at index 3")
    rejects(R.compare_samin, tiny, levels[:-1], match=r"samin: nlev")
