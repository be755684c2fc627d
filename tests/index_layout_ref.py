"""The layouts an index open derives in HBM (dicey_amd/csrc/index.hip derive_layouts; described in devfm.hpp FmView), restated from the
text bytes alone in plain numpy: no FM-index, no backward search, no rank structure.  The suffix array is a prefix-doubling sort of
the bytes; everything else is counted, sliced or looked up from the text and that array.  This module is the specification of the
layouts: tests/test_gpu_index_layout.py reads every layout back from the device (dgx_index_layout, development build) and holds it
against the model entry by entry, tests/test_index_layout_host.py holds the model against brute force and shows that every
comparer rejects the harmless-looking faults (a spurious filter bit, an escape bit that is always set, ...).

Every comparison is an exact integer comparison.  A comparer raises AssertionError("<layout>: first difference at index i ...").
"""
import random

import numpy as np

U32 = np.uint32
U64 = np.uint64
PLV_LINE, MAXPLV, MAXLEV = 448, 8, 10
SAX_POST_OFF, SAX_POST_N, SAX_ESCAPE = 16, 13, 0x80000000
WIDE = 0x80000000

CODE3 = np.full(256, 7, np.uint8)  # pre5 / sax / the K-mer codes: 0..3 = A,C,G,T, 7 = anything else
for _i, _c in enumerate(b"ACGT"):
    CODE3[_c] = _i
CODE_OF_BYTE = np.full(256, 7, np.uint8)  # devfm.hpp code_of_byte: the Occ planes
for _c, _v in ((65, 0), (67, 1), (71, 2), (84, 3), (78, 4), (10, 5), (0, 6)):
    CODE_OF_BYTE[_c] = _v

# ---------------------------------------------------------------------------------------------------------------------------
# The texts.  The first three are tests/test_gpu_index_open.py's (make_genome(seed, sequences, length)): two walks / sorted suffix
# array / one and two prefix levels.  "wide" is crafted: the default table order for it is K = 9, A^9 occurs 65536 times (the
# smallest wide table entry) and C^9 65535 times (the largest narrow one).
# ---------------------------------------------------------------------------------------------------------------------------
GENOMES = {"n40k": (211, 2, 20000), "n180k": (212, 3, 60000), "n300k": (213, 3, 100000)}
WIDE_A_RUN, WIDE_C_RUN = 65535 + 9, 65534 + 9


def _random_acgt(rng, length, not_first=None, not_last=None):
    """random A/C/G/T, no homopolymer longer than 5"""
    s = []
    while len(s) < length:
        c = rng.choice("ACGT")
        if len(s) == 0 and c == not_first:
            continue
        if len(s) == length - 1 and c == not_last:
            continue
        if len(s) >= 5 and all(x == c for x in s[-5:]):
            continue
        s.append(c)
    return "".join(s)


def wide_sequences():
    rng = random.Random(214)
    r = lambda n, **kw: _random_acgt(rng, n, **kw)  # noqa: E731
    first = r(1500) + "N" + r(700) + "NN" + r(900, not_last="A") + "A" * WIDE_A_RUN + r(1200, not_first="A") + "N" * 63 + r(800)
    short = "ACGTA"  # shorter than any table order
    last = r(1000, not_last="C") + "C" * WIDE_C_RUN + r(1100, not_first="C") + "N" * 64 + r(500) + "R" + r(600) + "N" * 65 + r(1500)
    return [first, short, last]


def text_of(name):
    """the bytes `dicey index` would see (conftest.genome_text) and the sequences"""
    if name == "wide":
        seqs = wide_sequences()
    else:
        from conftest import make_genome
        seqs = make_genome(*GENOMES[name])
    return ("\n".join(seqs) + "\n").encode(), seqs


TEXT_NAMES = list(GENOMES) + ["wide"]


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def suffix_array(full: bytes) -> np.ndarray:
    """prefix doubling over text + b"\\0": unsigned byte order, the sentinel (the only 0) smallest"""
    s = np.frombuffer(full, np.uint8)
    n = len(s)
    assert n and s[-1] == 0 and not (s[:-1] == 0).any()
    rank = np.unique(s, return_inverse=True)[1].astype(np.int64)  # dense: every rank stays below n
    k = 1
    while True:
        second = np.zeros(n, np.int64)  # 0 = past the end, below every rank + 1
        if k < n:
            second[:n - k] = rank[k:] + 1
        key = rank * (n + 1) + second
        order = np.argsort(key, kind="stable")
        ks = key[order]
        new = np.concatenate(([0], np.cumsum(ks[1:] != ks[:-1])))
        rank = np.empty(n, np.int64)
        rank[order] = new
        if new[-1] == n - 1:
            return order.astype(np.int64)
        k *= 2


def plv_sizes(n):
    """index_plan.hpp plan::plv_sizes"""
    xs, x = [], 1 << 16
    while x < n and len(xs) < MAXPLV:
        xs.append(x)
        x <<= 2
    return xs


def default_orders(n):
    """index_plan.hpp plan::table_orders on a device with room and no switches: K = ceil(log4 n) in [8, 16], K2 = K + 2"""
    K = 8
    while K < 16 and (1 << (2 * K)) < n:
        K += 1
    return K, K + 2


def _pack64(bits):
    """uint8 0/1 array whose length is a multiple of 64 -> u64 words, bit j of word w = bits[64 w + j]"""
    return np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def popcount(words):
    return int(np.bitwise_count(words).sum())


def filter_address(code, k, s):
    """bit address of a k-mer code in the filter copy whose in-line bits are code bits [s, s + 9) (devfm.hpp kf_test)"""
    code = np.asarray(code, np.uint64)
    s64 = U64(s)
    line = (code & ((U64(1) << s64) - U64(1))) | ((code >> (s64 + U64(9))) << s64)
    inl = (code >> s64) & U64(511)
    return line * U64(512) + inl


class Model:
    def __init__(self, text: bytes):
        self.text = text
        self.full = text + b"\0"
        self.s = np.frombuffer(self.full, np.uint8)
        self.n = len(self.full)
        self.sa = suffix_array(self.full)
        self._cache = {}

    def _memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    # ---- Occ blocks, C4 ----
    def bwt_codes(self):
        return self._memo("bwt", lambda: CODE_OF_BYTE[self.s[self.sa - 1]])  # sa == 0 -> s[-1], the sentinel

    def occ(self):
        """(cnt u32[nblk][4]: A/C/G/T in BWT[0, 128 b); planes u64[nblk][3][2]; mask u64[nblk][2]: the positions below n)"""
        def make():
            n, codes = self.n, self.bwt_codes()
            nblk = (n >> 7) + 1
            cnt = np.zeros((nblk, 4), U32)
            for c in range(4):
                cum = np.concatenate(([0], np.cumsum(codes == c)))
                cnt[:, c] = cum[np.arange(nblk) * 128]
            padded = np.zeros(nblk * 128, np.uint8)
            padded[:n] = codes
            planes = np.stack([_pack64((padded >> b) & 1).reshape(nblk, 2) for b in range(3)], axis=1)
            inside = np.zeros(nblk * 128, np.uint8)
            inside[:n] = 1
            return cnt, planes, _pack64(inside).reshape(nblk, 2)
        return self._memo("occ", make)

    def C4(self):
        """C[] of A, C, G, T: the symbols of text + sentinel below the letter; 0 when the letter is absent"""
        return [int((self.s < c).sum()) if (self.s == c).any() else 0 for c in b"ACGT"]

    def nrun_min(self):
        """the shortest run of 'N', capped at 64 (64 as well when there is none)"""
        isn = np.concatenate(([0], (self.s == ord("N")).astype(np.int8), [0]))
        d = np.diff(isn)
        lens = np.flatnonzero(d == -1) - np.flatnonzero(d == 1)
        return int(min(64, lens.min())) if len(lens) else 64

    # ---- k-mers ----
    def kmers(self, k):
        """per text position: valid (k characters of A/C/G/T from here, the sentinel not among them) and the code, first character on
        top, i.e. the last one in the low bits"""
        def make():
            n, c = self.n, CODE3[self.s]
            bad = np.where(c > 3, np.arange(n), n)
            nxt_bad = np.minimum.accumulate(bad[::-1])[::-1]  # s[n - 1] is the sentinel: always a stop
            valid = nxt_bad - np.arange(n) >= k
            padded = np.concatenate((c & 3, np.zeros(k, np.uint8))).astype(np.uint64)
            code = np.zeros(n, np.uint64)
            for j in range(k):
                code = code * U64(4) + padded[j:j + n]
            return valid, code
        return self._memo(("kmers", k), make)

    def present_codes(self, k):
        def make():
            valid, code = self.kmers(k)
            return np.unique(code[valid])
        return self._memo(("present", k), make)

    def ktab(self, K, with_pre5=True):
        """the table, decoded as devfm.hpp ktab_decode does: lo, width, wide (width >= 65536), pre_first = pre5[lo] & 0x7FFF for non-empty
        narrow entries when pre5 was built, 0x7FFF for the other narrow ones, 0xFFFFFFFF (not carried) for wide ones"""
        def make():
            valid, code = self.kmers(K)
            v_sa, c_sa = valid[self.sa], code[self.sa]
            idx = np.flatnonzero(v_sa)
            cs = c_sa[idx]
            first = np.concatenate(([True], (cs[1:] != cs[:-1]) | (idx[1:] != idx[:-1] + 1)))[:len(idx)]  # run boundaries in SA order
            starts = np.flatnonzero(first)
            codes, lo = cs[starts], idx[starts]
            hi = idx[np.concatenate((starts[1:], [len(idx)])).astype(np.int64)[:len(starts)] - 1] + 1
            assert len(np.unique(codes)) == len(codes), "suffixes that share a valid K-mer are neighbours in the suffix array"
            E = 1 << (2 * K)
            tlo, width = np.zeros(E, U32), np.zeros(E, U32)
            tlo[codes] = lo
            width[codes] = hi - lo
            wide = width >= 65536
            pre = np.full(E, 0x7FFF, U32)
            if with_pre5:
                pre[codes] = self.pre5()[lo].astype(U32) & U32(0x7FFF)
            pre[wide] = 0xFFFFFFFF
            return tlo, width, wide, pre
        return self._memo(("ktab", K, with_pre5), make)

    def filter_copy(self, k, s):
        """u32 words of the presence filter of order k in the copy whose in-line bits are code bits [s, s + 9)"""
        def make():
            addr = np.sort(filter_address(self.present_codes(k), k, s))
            words = np.zeros((1 << (2 * k)) >> 5, U32)
            if len(addr):
                w, bit = (addr >> U64(5)).astype(np.int64), U32(1) << (addr & U64(31)).astype(U32)
                starts = np.flatnonzero(np.concatenate(([True], w[1:] != w[:-1])))
                words[w[starts]] = np.bitwise_or.reduceat(bit, starts)
            return words
        return self._memo(("kf", k, s), make)

    # ---- pre5, sax ----
    def pre5(self):
        def make():
            c = np.concatenate((np.full(5, 7, np.uint8), CODE3[self.s])).astype(np.uint16)  # c[5 + p] = code of T[p]; 7 before the text
            v = np.zeros(self.n, np.uint16)
            for k in range(1, 6):
                v |= c[5 + self.sa - k] << np.uint16(3 * (k - 1))
            return v
        return self._memo("pre5", make)

    def sax(self):
        """(pos u32[n], esc bool[n], ctx u32[n]): ctx = the 30 context bits, meaningful where esc is False"""
        def make():
            n, p = self.n, self.sa
            c = np.concatenate((np.full(2, 7, np.uint8), CODE3[self.s], np.full(SAX_POST_OFF + SAX_POST_N, 7, np.uint8))).astype(U32)
            c1, c2 = c[2 + p - 1], c[2 + p - 2]
            esc = (c1 > 3) | (c2 > 3)
            ctx = (c1 & U32(3)) | ((c2 & U32(3)) << U32(2))
            for j in range(SAX_POST_N):
                cj = c[2 + p + SAX_POST_OFF + j]  # 7 outside the text; T[n - 1], the sentinel, is 7 by itself
                esc |= cj > 3
                ctx |= (cj & U32(3)) << U32(4 + 2 * j)
            return p.astype(U32), esc, ctx
        return self._memo("sax", make)

    # ---- prefix levels ----
    def plv(self, x):
        """(dir u64[nlines][8]: the count before the line and seven words of flags "SA[i] < x", zero at i >= n; idx: the flagged i)"""
        def make():
            nlines = self.n // PLV_LINE + 1
            flags = np.zeros(nlines * PLV_LINE, np.uint8)
            flags[:self.n] = self.sa < x
            words = _pack64(flags).reshape(nlines, 7)
            per_line = flags.reshape(nlines, PLV_LINE).sum(axis=1, dtype=np.uint64)
            before = np.concatenate(([0], np.cumsum(per_line)[:-1])).astype(np.uint64)
            return np.concatenate((before[:, None], words), axis=1), np.flatnonzero(flags)
        return self._memo(("plv", x), make)

    # ---- block minima ----
    def samin(self):
        """levels 1 .. nlev - 1 with their 0xFFFFFFFF padding out to ((nout + 7) & ~7) + 8 entries"""
        def make():
            out, prev = [], self.sa.astype(U32)
            while len(prev) > 8 and len(out) + 1 < MAXLEV:
                nout = (len(prev) + 7) // 8
                npad = ((nout + 7) & ~7) + 8
                body = np.full(nout * 8, 0xFFFFFFFF, U32)
                body[:len(prev)] = prev
                lv = np.full(npad, 0xFFFFFFFF, U32)
                lv[:nout] = body.reshape(nout, 8).min(axis=1)
                out.append(lv)
                prev = lv[:nout]
            return out
        return self._memo("samin", make)


# ---------------------------------------------------------------------------------------------------------------------------
# numpy emulation of the three packed value formats (what the kernels store), from the model's decoded values
# ---------------------------------------------------------------------------------------------------------------------------
def pack_ktab(lo, width, pre_first):
    """k_ktab_pack: (lo, width | pre_first << 16) below 2^16, (lo, 0x80000000 | width) from 2^16 on"""
    width = width.astype(U32)
    y = np.where(width >= 65536, U32(WIDE) | width, width | ((pre_first.astype(U32) & U32(0x7FFF)) << U32(16)))
    return np.stack((lo.astype(U32), y.astype(U32)), axis=1)


def pack_sax(pos, esc, ctx):
    """k_pre5: {position, context word | bit 31 when escaped}"""
    return np.stack((pos.astype(U32), np.where(esc, ctx | U32(SAX_ESCAPE), ctx).astype(U32)), axis=1)


def pack_plv_dir(sa, n, x):
    """k_plv_bits + k_plv_fill, line by line: {count before, seven ballots of i < n && SA[i] < x}"""
    nlines = n // PLV_LINE + 1
    out = np.zeros((nlines, 8), U64)
    total = 0
    for line in range(nlines):
        out[line, 0] = total
        for j in range(7):
            w = 0
            for lane in range(64):
                i = line * PLV_LINE + 64 * j + lane
                if i < n and sa[i] < x:
                    w |= 1 << lane
            out[line, 1 + j] = w
            total += bin(w).count("1")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# comparers: device arrays (as numpy) against the model
# ---------------------------------------------------------------------------------------------------------------------------
def _same(name, got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s%s: %s entries, the model has %s" % (name, what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[0])
        raise AssertionError("%s%s: first difference at index %d: device %s, model %s" % (name, what, i, got[i], want[i]))


def compare_occ(model, raw, verbose=True):
    """raw: the blocks as u64[nblk][8] — {cnt0 | cnt1 << 32, cnt2 | cnt3 << 32, pl[0][0], pl[0][1], pl[1][0], ...}"""
    cnt, planes, mask = model.occ()
    raw = np.asarray(raw, U64).reshape(-1, 8)
    assert len(raw) == len(cnt), "occ: %d blocks, the model has %d" % (len(raw), len(cnt))
    got_cnt = np.stack((raw[:, 0] & U64(0xFFFFFFFF), raw[:, 0] >> U64(32), raw[:, 1] & U64(0xFFFFFFFF), raw[:, 1] >> U64(32)), axis=1)
    _same("occ", got_cnt, cnt.astype(U64), " counts")
    got_pl = raw[:, 2:].reshape(-1, 3, 2)
    _same("occ", got_pl & mask[:, None, :], planes, " planes")
    if verbose:
        tail = got_pl[-1] & ~mask[-1][None, :]
        print("occ: the last block's plane bits at positions >= n (not asserted):", [hex(int(v)) for v in tail.reshape(-1)])


def decode_ktab(raw):
    """devfm.hpp ktab_decode on uint32[E][2]"""
    raw = np.asarray(raw, U32).reshape(-1, 2)
    y = raw[:, 1]
    wide = (y >> U32(31)) != 0
    width = np.where(wide, y & U32(0x7FFFFFFF), y & U32(0xFFFF))
    pre = np.where(wide, U32(0xFFFFFFFF), (y >> U32(16)) & U32(0x7FFF))
    return raw[:, 0], width, wide, pre


def compare_ktab(model, K, raw, with_pre5=True):
    lo, width, wide, pre = model.ktab(K, with_pre5)
    glo, gwidth, gwide, gpre = decode_ktab(raw)
    _same("ktab", gwidth, width, " width")
    _same("ktab", gwide, wide, " wide flag")
    _same("ktab", glo, lo, " lo")
    _same("ktab", gpre, pre, " pre_first")


def filter_code_of_address(addr, k, s):
    """the inverse of filter_address"""
    addr = np.asarray(addr, np.uint64)
    s64 = U64(s)
    line, inl = addr >> U64(9), addr & U64(511)
    return (line & ((U64(1) << s64) - U64(1))) | (inl << s64) | ((line >> s64) << (s64 + U64(9)))


def filter_yes_codes(words, k, s):
    """the sorted codes the copy answers "present" for — every other code 0 .. 4^k - 1 it answers "absent" for: with the sets of two
    copies equal, the two answer EVERY code alike"""
    words = np.asarray(words, "<u4")
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    w, b = np.nonzero(bits)
    return np.sort(filter_code_of_address(nz[w].astype(np.uint64) * U64(32) + b.astype(np.uint64), k, s))


def compare_filter(model, name, k, nr, s, pick, copies):
    """copies: the nr device copies as u32 words"""
    assert 1 <= nr <= 4 and len(copies) == nr, "%s: %d copies" % (name, nr)
    for t in range(32):
        assert ((pick >> (2 * t)) & 3) < nr, "%s: pick names copy %d at window position %d, there are %d" % (name, (pick >> (2 * t)) & 3, t, nr)
    present = model.present_codes(k)
    answers0 = None
    for r in range(nr):
        assert s[r] + 9 <= 2 * k, "%s copy %d: in-line bits [%d, %d) of a %d-bit code" % (name, r, s[r], s[r] + 9, 2 * k)
        words = np.asarray(copies[r], "<u4")
        assert len(words) == (1 << (2 * k)) >> 5, "%s copy %d: %d words" % (name, r, len(words))
        got = popcount(words)
        assert got == len(present), "%s copy %d: %d bits set, the text has %d distinct valid %d-mers" % (name, r, got, len(present), k)
        _same("%s copy %d (s = %d)" % (name, r, s[r]), words, model.filter_copy(k, s[r]), " words")
        answers = filter_yes_codes(words, k, s[r])
        if answers0 is None:
            answers0 = answers
        elif not np.array_equal(answers, answers0):
            code = int(np.setxor1d(answers, answers0)[0])
            raise AssertionError("%s copy %d: answers code %d differently from copy 0" % (name, r, code))


def compare_pre5(model, raw):
    _same("pre5", np.asarray(raw, np.uint16), model.pre5())


def compare_sax_records(name, raw, pos, esc, ctx):
    raw = np.asarray(raw, U32).reshape(-1, 2)
    _same(name, raw[:, 0], pos, " position")
    _same(name, (raw[:, 1] & U32(SAX_ESCAPE)) != 0, esc, " escape bit")
    keep = ~esc
    if not np.array_equal(raw[keep, 1], ctx[keep]):
        i = int(np.flatnonzero(keep)[np.flatnonzero(raw[keep, 1] != ctx[keep])[0]])
        raise AssertionError("%s context: first difference at index %d: device %#x, model %#x" % (name, i, raw[i, 1], ctx[i]))


def compare_sax(model, raw):
    compare_sax_records("sax", raw, *model.sax())


def compare_plv(model, level, x, dir_raw, rec_raw, sax_raw=None):
    want_dir, idx = model.plv(x)
    _same("plv[%d] dir (x = %d)" % (level, x), np.asarray(dir_raw, U64).reshape(-1, 8), want_dir)
    pos, esc, ctx = model.sax()
    rec = np.asarray(rec_raw, U32).reshape(-1, 2)
    assert len(rec) == len(idx), "plv[%d] rec: %d records, %d suffixes lie below %d" % (level, len(rec), len(idx), x)
    compare_sax_records("plv[%d] rec" % level, rec, pos[idx], esc[idx], ctx[idx])
    if sax_raw is not None:  # the records are copies of the device's own sax entries, escaped low bits included
        _same("plv[%d] rec against sax" % level, rec, np.asarray(sax_raw, U32).reshape(-1, 2)[idx])


def compare_samin(model, levels):
    """levels: the device's levels 1 .. nlev - 1, each with its padding"""
    want = model.samin()
    assert len(levels) == len(want), "samin: nlev %d, the model has %d" % (len(levels) + 1, len(want) + 1)
    for j, (g, w) in enumerate(zip(levels, want)):
        _same("samin[%d]" % (j + 1), np.asarray(g, U32), w)
