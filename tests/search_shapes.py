"""Inputs for the site stage of `dicey search` (dicey_amd/csrc/search.hip) at the primer and window shapes its other tests never
produce: primers over 30 nt (second trace word of the wave alignment), self-complementary primers and windows (the symmetry
correction), primers of 58-60 nt (the sequential kernel as the whole path), distance 2, the wide traceback kernel, primers thal()
refuses, windows cut by sequence ends, N runs and IUPAC letters, and cuts that sit exactly on a site's Tm.

Everything comes from seeds; nothing here touches a GPU or the library under test.  genome() is one text of five sequences with the
features planted, cases() the named primer batches with their search parameters, expected() what the oracle (restated silica.h over
the reference's own thal(), oracle/_ref) answers for a case.  tests/test_search_shapes_host.py asserts, from the oracle alone, that
every case still has the property it exists for; tests/test_gpu_search_shapes.py compares the library and the binary with it.

The text has 530 kb and not the megabases of a chromosome arm: the site stage sees windows of at most 70 nt around a hit, so the
text's size only changes how many chance hits a short k-mer has, and the oracle pays a reference thal() call for each of them."""
import os
import random
import struct
import tempfile

import oracle_lib as O
from conftest import revcomp

NAMES = ["chrA", "chrB", "chrC", "chrD", "chrE"]
LENGTHS = [90001, 70003, 60000, 50017]        # chrE is the planted family of many_hits_57, 5 200 copies of 50 nt
FAMILY = 5200
N_RUN, R_AT, Y_AT = 30000, 40000, 40200      # in chrC: "NNNNNNNN", one 'R', one 'Y'
_memo = {}


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _mutate(rng, s, i):
    return s[:i] + rng.choice([c for c in "ACGT" if c != s[i]]) + s[i + 1:]


def _pal(rng, n):
    h = _rand(rng, n // 2)
    return h + revcomp(h)


def genome():
    """{"seqs", "names", "text", "seqlen", "cases"}: built once per process"""
    if "g" in _memo:
        return _memo["g"]
    rng = random.Random(20261)
    seqs = [list(_rand(rng, n)) for n in LENGTHS]
    cursor = [0, 1000, 0, 0]

    def plant(s, ci=1):      # every planted piece sits in chrB between 150 nt of the random text
        at = cursor[ci]
        seqs[ci][at:at + len(s)] = list(s)
        cursor[ci] = at + len(s) + 150
        return at
    cases = {}
    hd0 = dict(kmer=15, distance=0, hamming=True, cutTemp=0.0)

    # ---- palindromes: kind -> primers; at Hamming distance 0 the window of a hit is the primer's own site, nothing more
    kinds = {"both": [], "odd": [], "central": [], "window_only": [], "with_n": []}
    for n in list(range(16, 42, 2)) * 2:
        p = _pal(rng, n)
        plant(p)
        kinds["both"].append(p)
    for n in range(17, 37, 2):                       # odd length: a centre base between the two halves
        h = _rand(rng, n // 2)
        p = h + rng.choice("ACGT") + revcomp(h)
        plant(p)
        kinds["odd"].append(p)
    for n in range(22, 42, 2):                       # one of the two centre bases no longer pairs with the other
        p = _pal(rng, n)
        p = p[:n // 2] + p[n // 2 - 1] + p[n // 2 + 1:]       # x x: no base is its own complement
        plant(p)
        kinds["central"].append(p)
    for n in range(22, 42, 2):                       # the site is a palindrome, the primer differs from it in its 5' overhang
        p = _pal(rng, n)
        plant(p)
        kinds["window_only"].append(_mutate(rng, p, rng.randrange(0, n - 15)))
    for i, n in enumerate([34, 36, 38, 40, 40] * 2):  # N at two mirrored places of the overhang: in the primer alone, then in the site too
        p = _pal(rng, n)
        a = rng.randrange(15, n - 15)
        pn = p[:a] + "N" + p[a + 1:]
        pn = pn[:n - 1 - a] + "N" + pn[n - a:]
        plant(p if i < 5 else pn)
        kinds["with_n"].append(pn)
    cases["palindromes"] = dict(primers=[p for k in kinds.values() for p in k], kinds={k: len(v) for k, v in kinds.items()}, **hd0)
    cases["palindromes_edit1"] = dict(primers=list(kinds["both"]), kmer=15, distance=1, hamming=False, cutTemp=0.0)
    # 58 + 3 * 1 + 2 > 62: at distance 1 these are too long for the wave kernel, and with Hamming the window still is the site alone,
    # so the sequential kernel's own symmetry test answers true for both oligos
    longpal = [_pal(rng, n) for n in (58, 60, 60, 58, 60, 58)]
    for p in longpal:
        plant(p)
    cases["palindromes_58_60"] = dict(primers=longpal, kmer=15, distance=1, hamming=True, cutTemp=0.0)

    # ---- distance 2: copies of six 60-nt pieces with one and two edits inside what a primer's k-mer covers
    d2src = []
    for _ in range(6):
        piece = _rand(rng, 60)
        plant(piece)
        d2src.append(piece)
        for nedit in (1, 2, 2):
            c = piece
            for _e in range(nedit):
                i = rng.randrange(32, 58)
                r = rng.random()
                c = _mutate(rng, c, i) if r < 0.5 else (c[:i] + c[i + 1:] if r < 0.75 else c[:i] + rng.choice("ACGT") + c[i:])
            plant(c)
    seqs[2][N_RUN:N_RUN + 8] = list("N" * 8)
    seqs[2][R_AT] = "R"
    seqs[2][Y_AT] = "Y"
    seqs = ["".join(s) for s in seqs]
    # the family: one 30-nt unit between 10 nt of random text on either side, FAMILY times; every 15-mer of the unit occurs FAMILY times
    frng = random.Random(20262)
    unit = _rand(frng, 30)
    copies = [_rand(frng, 10) + unit + _rand(frng, 10) for _ in range(FAMILY)]
    seqs.append("".join(copies))

    def cut(ci, n, lo=2000, hi=None, strand=None):
        s = seqs[ci]
        while True:
            a = rng.randrange(lo, (hi or len(s) - 2000) - n)
            p = s[a:a + n]
            if set(p) <= set("ACGT"):
                break
        fw = (rng.random() < 0.5) if strand is None else strand
        return p if fw else revcomp(p)

    # ---- 31..57 nt: windows of 33 nt and more at distance 1, both strands; every third primer with a mismatch in its first nt
    long_p = []
    for n in range(31, 58):
        for strand in (True, False, True, False):
            p = cut(0, n, strand=strand)
            if len(long_p) % 3 == 2:
                p = _mutate(rng, p, 0)       # outside the last 15 and the last 30 nt alike
            long_p.append(p)
    cases["len31_57"] = dict(primers=long_p, kmer=15, distance=1, hamming=False, cutTemp=45.0)
    cases["len31_57_k30"] = dict(primers=long_p, kmer=30, distance=1, hamming=False, cutTemp=45.0)
    cases["k_plen_minus_1"] = dict(primers=[cut(0, 41, strand=i % 2 == 0) for i in range(8)], kmer=40, distance=1, hamming=False, cutTemp=45.0)

    # ---- 58..60 nt: beyond what the wave kernel takes, so the sequential kernel does the whole batch
    seq_p = [cut(0, n, strand=st) for n in (58, 59, 60) for st in (True, False, True, False)]
    cases["sequential_58_60_d0"] = dict(primers=seq_p, kmer=15, distance=0, hamming=False, cutTemp=45.0)
    cases["sequential_58_60_d1"] = dict(primers=seq_p, kmer=15, distance=1, hamming=False, cutTemp=45.0)
    short_p = [cut(0, 20) for _ in range(10)]
    cases["sequential_mixed"] = dict(primers=short_p[:5] + [seq_p[-1]] + short_p[5:], kmer=15, distance=1, hamming=False, cutTemp=45.0)

    # ---- 50..57 nt at edit distance 1 and a short k: the longest windows the wave kernel keeps for itself
    hb = [cut(0, n, strand=st) for n in range(50, 58) for st in (True, False)]
    cases["handback_k10"] = dict(primers=hb, kmer=10, distance=1, hamming=False, cutTemp=45.0)
    cases["handback_k11"] = dict(primers=hb, kmer=11, distance=1, hamming=False, cutTemp=45.0)
    cases["handback_k12"] = dict(primers=hb, kmer=12, distance=1, hamming=False, cutTemp=45.0)
    cases["handback_k13"] = dict(primers=hb, kmer=13, distance=1, hamming=False, cutTemp=45.0)

    # ---- many hits: 20-mers whose last 15 nt are a 15-mer of the unit.  Primer j carries the 5 nt in front of it in copy 100 j (its one
    # site over the cut, with chance matches) when the 15-mer starts the unit, else 5 nt that do not match the unit.  The longest primer
    # of a batch sets the hits per k_site launch (chunk_of): one 57-mer / 60-mer from chrA, LAST, so that its hit lies in the last launch
    def fam_primer(j):
        o = (j % 4) * 5 if j % 4 else 0
        if o == 0:
            return copies[100 * j][5:10] + unit[:15]
        return "".join({"A": "C", "C": "A", "G": "T", "T": "G"}[c] for c in unit[o - 5:o]) + unit[o:o + 15]
    # The case is reduced to the cheapest batch that spans two launches: a reference thal() call costs the oracle about 0.2 ms for a
    # 20-mer, so the 110 000 hits a batch on the sequential path needs, or the 153 000 a batch of 20-mers alone needs, are 20-35 s of
    # host time in each of the two modules; 20 801 hits with one 57-mer are 4 s
    fam = [fam_primer(j) for j in range(4)]
    cases["many_hits_57"] = dict(primers=fam + [cut(0, 57, strand=True)], kmer=15, distance=0, hamming=False, cutTemp=50.0)

    # ---- distance 2
    def d2_primers(count):
        out = []
        for i in range(count):
            n = 18 + (i * 5) % 13      # 18..30
            p = d2src[i % 6][58 - n:58]
            out.append(p if i % 2 == 0 else revcomp(p))
        return out
    for k in (13, 15):
        cases["distance2_edit_k%d" % k] = dict(primers=d2_primers(4), kmer=k, distance=2, hamming=False, cutTemp=40.0)
        cases["distance2_hamming_k%d" % k] = dict(primers=d2_primers(8), kmer=k, distance=2, hamming=True, cutTemp=40.0)
    cases["distance2_capped"] = dict(primers=[revcomp(d2src[1][28:58])], kmer=28, distance=2, hamming=False, cutTemp=40.0)

    # ---- (60 + 6 + 3) * 60 > 4096 cells: the sequential kernel with the wide traceback
    t0 = cut(0, 60, strand=True)
    t2 = cut(0, 60, strand=False)
    t2 = _mutate(rng, _mutate(rng, t2, 20), 41)
    cases["trace2600"] = dict(primers=[t0, cut(0, 60, strand=False), t2], kmer=59, distance=2, hamming=True, cutTemp=45.0,
                              maxNeighborhood=20000)

    # ---- primers thal() refuses (both oligos over 60 nt), and one the library does not store
    keep3 = [cut(0, 20) for _ in range(3)]
    cases["refused_base"] = dict(primers=keep3, kmer=15, distance=1, hamming=False, cutTemp=45.0)
    _memo["refused"] = {"p61": cut(0, 61, strand=True), "p64": cut(0, 64, strand=False), "p65": cut(0, 65, strand=True)}

    # ---- windows cut short or holding other letters than A/C/G/T: 30-nt primers, the searched 15 nt 0..5 nt away from the feature
    dirty = []
    for ci in (0, 1, 2, 3, 4):
        s = seqs[ci]
        for j in range(6):
            if ci < 4:
                dirty.append(_rand(rng, 15) + s[j:j + 15])                              # start of a sequence (chrA: of the text)
            if ci != 3:
                dirty.append(_rand(rng, 15) + revcomp(s[len(s) - 15 - j:len(s) - j]))   # end of a sequence (chrE: of the text)
    s = seqs[2]
    for at, width in ((N_RUN, 8), (R_AT, 1), (Y_AT, 1)):
        for j in range(6):
            b = at + width + j
            dirty.append((s[b - 15:b] if j % 2 == 0 else _rand(rng, 15)) + s[b:b + 15])  # the feature inside the 5' overhang's window
            e = at - j
            dirty.append(revcomp(s[e - 15:e + 15]))                                     # the same from the other strand
    for i in range(4):                                                                  # N inside the searched k-mer
        p = cut(2, 30, lo=2000, hi=25000)
        dirty.append(p[:18 + 3 * i] + "N" + p[19 + 3 * i:])
    cases["dirty_windows"] = dict(primers=dirty, kmer=15, distance=1, hamming=False, cutTemp=10.0)

    # ---- primer length equal to k: no overhang at all, the window is the hit (plus the context of edit distance 1).  The reference's
    # FASTA reader takes only records longer than k, so the oracle runs these with that one comparison relaxed (expected(): accept_len_k)
    lenk = [cut(2, 15, lo=2000, hi=25000, strand=i % 2 == 0) for i in range(6)] + [seqs[1][:15], revcomp(seqs[3][-15:])]
    cases["len_equals_k_d0"] = dict(primers=lenk, kmer=15, distance=0, hamming=False, cutTemp=20.0, accept_len_k=True)
    cases["len_equals_k_d1"] = dict(primers=lenk, kmer=15, distance=1, hamming=False, cutTemp=20.0, accept_len_k=True)

    # ---- a dozen 22-mers with one site each: the cut is then put on, just below and just above each site's Tm
    cases["cut_edge"] = dict(primers=[cut(3, 22) for _ in range(12)], kmer=15, distance=0, hamming=False, cutTemp=45.0)

    text = ("\n".join(seqs) + "\n").encode()
    g = {"seqs": seqs, "names": NAMES, "text": text, "seqlen": [len(x) + 1 for x in seqs], "cases": cases}
    _memo["g"] = g
    return g


def cases():
    return genome()["cases"]


CASE_NAMES = ["palindromes", "palindromes_edit1", "palindromes_58_60", "many_hits_57", "len_equals_k_d0",
              "len_equals_k_d1", "handback_k11", "handback_k12", "len31_57", "len31_57_k30", "k_plen_minus_1", "sequential_58_60_d0",
              "sequential_58_60_d1", "sequential_mixed", "handback_k10", "handback_k13", "distance2_edit_k13", "distance2_hamming_k13",
              "distance2_edit_k15", "distance2_hamming_k15", "distance2_capped", "trace2600", "refused_base", "dirty_windows", "cut_edge"]


def refused_primers():
    genome()
    return _memo["refused"]


def as_stored(p):
    """what the reference keeps of a primer: upper case, every other letter than A/C/G/T replaced by N (util.h:208-219)"""
    return "".join(c if c in "ACGT" else "N" for c in p.upper())


def fasta(primers):
    return "".join(">p%d\n%s\n" % (i, p) for i, p in enumerate(primers))


def oracle_kw(case, **over):
    kw = {k: case[k] for k in ("kmer", "distance", "hamming", "cutTemp", "maxNeighborhood", "max_locations") if k in case}
    kw.update(over)
    return kw


def library_kw(case, **over):
    kw = oracle_kw(case, **over)
    return dict(kmer=kw["kmer"], distance=kw["distance"], hamming=kw["hamming"], cut_temp=kw["cutTemp"],
                max_neighborhood=kw.get("maxNeighborhood", 10000), max_locations=kw.get("max_locations", 10000))


def chunk_of(case):
    """hits per k_site launch as launch_site_stage sizes them: DP planes of the longest primer times the widest window, 16 bytes a cell,
    1 GB when the wave kernel does the work (only handed-back hits reach k_site), 6 GB when k_site does it all"""
    maxp = max(len(p) for p in case["primers"])
    wmax = maxp + 3 * case["distance"] + 2
    wave = maxp <= 62 and wmax <= 62
    return max(4096, ((1 << 30) if wave else (6 << 30)) // (16 * maxp * wmax + 1)), wave


def oracle_index():
    """the oracle's index of the text, written once per process"""
    if "ix" not in _memo:
        if O.ref_libs() is None:
            raise AssertionError("oracle/_ref is missing: __graft_entry__.build() compiles it (oracle/Makefile)")
        g = genome()
        import atexit
        import shutil
        d = tempfile.mkdtemp(prefix="search_shapes_")
        atexit.register(shutil.rmtree, d, True)
        path = os.path.join(d, "shapes.fm9")
        O.build_fm9(g["text"], path)
        _memo["ix"] = (O.Index(path), path)
    return _memo["ix"][0]


def bits(x):
    return struct.pack("<d", x)


def ref_match_temp(p):
    """the reference's thal(primer, reverse complement), silica.h:431-443"""
    import ctypes as C
    T, _ = O.ref_libs()
    T.ref_thal.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    t, a, b = C.c_double(), C.c_int(), C.c_int()
    T.ref_thal(p.encode(), revcomp(p).encode(), C.byref(t), C.byref(a), C.byref(b))
    return t.value


def expected(name, **over):
    """the oracle's answer for a case: {"json", "rc", "located", "pushed", "match_temp", "max_matches", "nbhd_warnings", "primers"}.
    pushed is the binding sites in the order of the reference's push_back calls, located every hit that reached thal()"""
    key = (name, tuple(sorted(over.items())))
    if key not in _memo:
        g = genome()
        case = g["cases"][name]
        prim = [as_stored(p) for p in case["primers"]]
        kw = oracle_kw(case, **over)
        O.lib().orc_search_accept_len_k(1 if case.get("accept_len_k") else 0)
        try:
            js, rc, located, pushed = oracle_index().search(g["seqlen"], g["names"], g["text"], fasta(case["primers"]), want_log=True, **kw)
        finally:
            O.lib().orc_search_accept_len_k(0)
        assert rc == 0, js[:300]
        per = {}
        for h in located:
            per[h[0]] = per.get(h[0], 0) + 1
        cap = kw.get("max_locations", 10000)
        _memo[key] = {"json": js, "rc": rc, "located": located, "pushed": pushed, "primers": prim,
                      "match_temp": [ref_match_temp(p) for p in prim] if not over else None,
                      "max_matches": [per.get(i, 0) >= cap for i in range(len(prim))],
                      "nbhd_warnings": js.count("Warning: Neighborhood size exceeds")}
    return _memo[key]


# ---- plain restatements, for counting what a case produced on the reference side --------------------------------------------------

def self_complementary(s):
    """symmetry_thermo (thal.h:1976-2010): even length, and wherever one of two mirrored letters is A/C/G/T the other is its
    complement; a pair of other letters (N N) passes"""
    if len(s) % 2:
        return False
    pair = {"A": "T", "T": "A", "C": "G", "G": "C"}
    for i in range(len(s) // 2):
        a, b = s[i], s[-1 - i]
        if (a in pair and pair[a] != b) or (b in pair and pair[b] != a):
            return False
    return True


def window(text, loc, mlen, strand, koff, ctx):
    """silica.h:478-500: (window, pre, post, pre_eff): ctx letters of context on both sides (edit distance; 0 for Hamming) plus the
    primer's 5' overhang koff on the left of a forward hit / the right of a reverse hit, clipped to the text, cut at '\\n'"""
    n = len(text) + 1            # the index text ends in the sentinel
    pre = post = ctx
    if strand:
        post += koff
    else:
        pre += koff
    pre = min(pre, loc)
    if loc + mlen + post > n:
        post = n - loc - mlen
    left = text[loc - pre:loc].decode("latin-1")
    right = text[loc + mlen:loc + mlen + post].decode("latin-1")
    if "\n" in left:
        left = left[left.rfind("\n") + 1:]
    if "\n" in right:
        right = right[:right.find("\n")]
    return left + text[loc:loc + mlen].decode("latin-1") + right, pre, post, len(left)


def hit_windows(name, **over):
    """(located hit, window, pre, post, pre_eff, chrpos) for every located hit of a case, the window rebuilt from the text"""
    g = genome()
    case = g["cases"][name]
    e = expected(name, **over)
    ctx = 0 if case["hamming"] else case["distance"]
    starts = [0]
    for n in g["seqlen"]:
        starts.append(starts[-1] + n)
    out = []
    for h in e["located"]:
        q, fr, loc, mlen, wlen, temp = h
        w, pre, post, pre_eff = window(g["text"], loc, mlen, fr, len(e["primers"][q]) - case["kmer"], ctx)
        assert len(w) == wlen, (name, h, w)
        ref = max(i for i in range(len(g["seqlen"])) if starts[i] <= loc)
        out.append((h, w, pre, post, pre_eff, loc - starts[ref]))
    return out
