"""Inputs for the verify stage of `dicey hunt` (dicey_amd/csrc/hunt_verify.hpp, band_bits.hpp; dispatch in hunt.hip run_batch): the
stage that turns a located hit into score, chromosome, start and the two alignment rows.  One arithmetic, nine launchable forms:
k_verify_memo<7|13, 1|4|8> (the bit-plane band, classes of hits shared through an LDS hash table), k_verify<1,true,24>,
<1,true,32>, <160,false>, <2200,false> (full matrix) with k_rows_to_ops / k_hits_to_compact behind them, and k_verify_long.

Everything comes from seeds; nothing here touches a GPU or the library under test.  genome() is one text of about 150 kb in five
sequences with everything planted, batches() the named query batches with their hunt parameters, expected() the oracle's hits of a
batch in push order, push_list() the same list rebuilt in Python (neighbourhood, locate, the loop of hunter.h:489-543) so that every
hit carries its text position, its kept string and its class: (kept string, pre_eff, post_eff, context bytes), the key under which
k_verify_memo lets hits share one alignment.  tests/test_verify_shapes_host.py asserts, from the oracle alone, that every batch still
has the property it exists for; tests/test_gpu_verify_shapes.py compares the library with it, hit by hit.

Batches
  ties     queries of 12-32 nt around a homopolymer run or a 2-/3-nt tandem repeat, each planted with one edit: substitution,
           deletion, insertion x first column, last column, inside the run, at the run's edge; flanks continue the run where that
           leaves the edit in place; every other query is given as its reverse complement.  Every edit but a substitution strictly
           inside the query has two or more optimal alignments (needle.h:105-131 picks horizontal, then vertical, then diagonal);
           a substitution inside the query has no second path of cost 1 through it (that would need two gaps), and is kept as
           the control.
  classes20 / classes14
           one 20-nt (14-nt) string planted F20 (F14) times between flanks that cycle through all 16 A/C/G/T pairs, N / R / Y on
           either side and at distance 2, '\\n' one and two characters away on either side (offset 0 and 1 of a sequence, ending 0
           and 1 before its end), the first position of the text (the 20-nt string) and the last one before the final separator
           (the 14-nt string).  classes20_d2 / classes14_d1 run each family at the other distance, so that both band widths see
           both ends of the text.  The queries are the
           string plus one inserted character (distance 1) / two edits away (distance 2), so every copy is a hit of every query
           and the flank decides score, start and rows.
  clean    160 20-mers cut from the background (a third with one substitution): a handful of hits per query.
  len*     the three edit kinds on queries whose longest is exactly 24, 25, 32 (distance 3: full matrix; distance 1: the band), 33,
           the two lengths either side of (maxlen + 3 d + 1) (maxlen + 1) == 32 * 160 at distance 1 and at distance 2, 255, 256, 300;
           the last three also at distance 2.  From distance 2 on every query is also planted as q[1] x q[2:] and q[0] x q[1] q[3:],
           where horizontal, vertical and diagonal moves tie on the optimal path.  Each with a forward-only Hamming variant (and a compact=False delivery in the GPU module).
  deep3 / deep4
           distance 3 and 4 on 12- to 15-nt queries: leading query-gap columns of 3 and 4, hits by the hundred.
Batches whose neighbourhoods exceed what the checker enumerates in seconds run with a small max_neighborhood: the reference then
searches the first strings of its walk (neighbors.h:47-83), the library must search the same ones, and the planted strings are taken
from that list."""
import os
import random
import tempfile

import oracle_lib as O
from conftest import revcomp

NAMES = ["vA", "vB", "vC", "vD", "vE"]
LENGTHS = [30011, 30000, 29989, 30002, 30017]
F20_BULK, F14_BULK = 300, 260
NBHD_SMALL = 2000            # max_neighborhood of the batches whose full neighbourhood the checker cannot enumerate in seconds
FULL_MATRIX_CELLS = 32 * 160  # hunt.hip: cells <= 32 * 160 selects k_verify<160, false>
MAX_QLEN = 255               # hunt_verify.hpp: longer queries take k_verify_long
CLASS_BATCHES = ["classes20", "classes14", "classes20_d2", "classes14_d1"]
_memo = {}


def cells(maxlen, d):
    """hunt.hip run_batch: the full matrix of the batch's longest query"""
    return (maxlen + 3 * d + 1) * (maxlen + 1)


def cells_edge(d):
    """the longest query length that still takes k_verify<160,false> at distance d, and the next one"""
    n = 33
    while cells(n + 1, d) <= FULL_MATRIX_CELLS:
        n += 1
    return n, n + 1


def kernel_of(maxlen, d):
    """hunt.hip run_batch: the verify kernel of a hunt batch from its longest query and its distance"""
    if maxlen <= 32 and d <= 2:
        return "k_verify_memo"
    if maxlen > MAX_QLEN:
        return "k_verify_long"
    if maxlen <= 24:
        return "k_verify<1,true,24>"
    if maxlen <= 32:
        return "k_verify<1,true,32>"
    return "k_verify<160,false>" if cells(maxlen, d) <= FULL_MATRIX_CELLS else "k_verify<2200,false>"


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _other(rng, *avoid):
    return rng.choice([c for c in "ACGT" if c not in avoid])


def nw_score(window, query):
    """needle() as hunt calls it (needle.h:59-138, AlignConfig<false,true>): rows = window, columns = query; match 0, mismatch and
    gaps -1; moves down column 0 and the last column are free"""
    n = len(query)
    prev = [-c for c in range(n + 1)]
    for r in range(1, len(window) + 1):
        cur = [0] * (n + 1)
        w = window[r - 1]
        for c in range(1, n + 1):
            cur[c] = max(prev[c - 1] - (w != query[c - 1]), prev[c] - (c != n), cur[c - 1] - 1)
        prev = cur
    return prev[n]


def rows_under(window, query, order):
    """needle() + hunt's column stripping with the three moves tried in `order` ("hvd" is needle.h:105-131): (refalign, queryalign,
    leading columns dropped)"""
    m, n = len(window), len(query)
    sc = [[0] * (n + 1) for _ in range(m + 1)]
    for c in range(n + 1):
        sc[0][c] = -c
    for r in range(1, m + 1):
        row, up, w = sc[r], sc[r - 1], window[r - 1]
        for c in range(1, n + 1):
            row[c] = max(up[c - 1] - (w != query[c - 1]), up[c] - (c != n), row[c - 1] - 1)
    r, c, ra, qa = m, n, [], []
    while r or c:
        ok = {"h": c > 0 and (r == 0 or sc[r][c] == sc[r][c - 1] - 1),
              "v": r > 0 and (c == 0 or sc[r][c] == sc[r - 1][c] - (c != n)),
              "d": r > 0 and c > 0 and sc[r][c] == sc[r - 1][c - 1] - (window[r - 1] != query[c - 1])}
        mv = next(x for x in order if ok[x])
        if mv == "h":
            c -= 1
            ra.append("-")
            qa.append(query[c])
        elif mv == "v":
            r -= 1
            ra.append(window[r])
            qa.append("-")
        else:
            r -= 1
            c -= 1
            ra.append(window[r])
            qa.append(query[c])
    ra, qa = ra[::-1], qa[::-1]
    last = max(i for i, x in enumerate(qa) if x != "-")
    lead = next(i for i, x in enumerate(qa) if x != "-")
    return "".join(ra[lead:last + 1]), "".join(qa[lead:last + 1]), lead


def _overlapping(hay, pat):
    k, at = 0, hay.find(pat)
    while at >= 0:
        k += 1
        at = hay.find(pat, at + 1)
    return k


# ---------------------------------------------------------------------------------------------------------------------- the text

FLANKS = ([("%s%s" % (o, a), "%s%s" % (b, p)) for (a, b), o, p in zip([(a, b) for a in "ACGT" for b in "ACGT"], "ACGT" * 4, "TGCA" * 4)] +
          [("AN", "CG"), ("CG", "NA"), ("NT", "GC"), ("TC", "GN"), ("GR", "TA"), ("AT", "RC"), ("CY", "AG"), ("GA", "YT"),
           ("RA", "CC"), ("TG", "AY")])


def genome():
    """{"seqs", "names", "text", "seqlen", "batches", "plants", "families"}: built once per process"""
    if "g" in _memo:
        return _memo["g"]
    rng = random.Random(20270)
    seqs = [list(_rand(rng, n)) for n in LENGTHS]
    cursor = [1000, 100, 100, 100, 100]          # vA[1000:] stays background: the clean queries are cut there
    regions = []                                  # (sequence, offset, planted string with its flanks)

    def put(ci, at, s):
        assert 0 <= at and at + len(s) <= len(seqs[ci])
        seqs[ci][at:at + len(s)] = list(s)
        regions.append((ci, at, s))

    def plant(ci, s, pre="", post=""):
        """s between the flanks pre / post and 24 nt of background; returns where s starts"""
        at = cursor[ci]
        put(ci, at, pre + s + post)
        cursor[ci] = at + len(pre) + len(s) + len(post) + 24
        assert cursor[ci] < len(seqs[ci]) - 200, "sequence %d is full" % ci
        return at + len(pre)
    batches, plants = {}, []

    def plant_case(batch, qi, kind, place, fw, s, pre, post, ci, distance):
        q = batches[batch]["queries"][qi]
        qq = q if fw else revcomp(q)
        at = plant(ci, s, pre, post)
        if kind == "ham":    # hunter.h:79-88: no context, position by position
            score = -sum(1 for a, b in zip(s, qq) if a != b)
        elif kind == "tie":  # the kept string is q[distance:], located `distance` characters into s: its context in front is s's own
            score = nw_score(s + post[:distance], qq)
        else:
            score = nw_score(pre[len(pre) - distance:] + s + post[:distance], qq)
        plants.append(dict(batch=batch, query=qi, kind=kind, place=place, strand="+" if fw else "-", seq=ci, at=at, planted=s,
                           score=score))

    # ---- the two families
    k20 = _rand(rng, 7) + "AAA" + _rand(rng, 10)
    k20 = k20[:6] + _other(rng, "A") + k20[7:10] + _other(rng, "A") + k20[11:]
    k14 = _rand(rng, 5) + "CC" + _rand(rng, 7)
    k14 = k14[:4] + _other(rng, "C") + k14[5:7] + _other(rng, "C") + k14[8:]
    fam = {"k20": dict(string=k20, at=[]), "k14": dict(string=k14, at=[])}
    # sequence starts and ends: offset 0 / 1, ending 0 / 1 before the end, each string also at offset 0 of a sequence that is not the
    # first and ending a sequence that is not the last; k20 opens the text, k14 closes it (one string only can do either: each family
    # is therefore run at both distances, classes20_d2 and classes14_d1 below, so that both band widths meet both ends of the text)
    edge = [("k20", 0, "start", ""), ("k14", 0, "end", ""), ("k14", 1, "start", "G"), ("k20", 1, "end", "T"), ("k14", 2, "start", ""),
            ("k20", 2, "end", ""), ("k20", 3, "start", "C"), ("k14", 3, "end", "A"), ("k20", 4, "start", ""), ("k14", 4, "end", "")]
    for name, ci, side, x in edge:
        s = fam[name]["string"]
        if side == "start":
            put(ci, 0, x + s)
            fam[name]["at"].append((ci, len(x)))
        else:
            put(ci, len(seqs[ci]) - len(s) - len(x), s + x)
            fam[name]["at"].append((ci, len(seqs[ci]) - len(s) - len(x)))
    for k in range(F20_BULK):
        pre, post = FLANKS[k % len(FLANKS)]
        fam["k20"]["at"].append((4, plant(4, k20, pre, post)))
    for k in range(F14_BULK):
        pre, post = FLANKS[(k * 7) % len(FLANKS)]
        fam["k14"]["at"].append((3, plant(3, k14, pre, post)))

    def both(qs):
        return [q if i % 2 == 0 else revcomp(q) for q in qs for i in range(2)]
    # the 20-nt string is each query with one character deleted: in front, behind, inside the AAA run, inside the random part
    x = _other(rng, k20[13], k20[14])
    batches["classes20"] = dict(queries=both(["A" + k20, k20 + "T", k20[:8] + "A" + k20[8:], k20[:14] + x + k20[14:]]),
                                kw=dict(distance=1, max_locations=5000), family="k20")
    # the 14-nt string is two edits away from each query
    s1, s2 = _other(rng, k14[3]), _other(rng, k14[10])
    x1, x2 = _other(rng, k14[8], k14[9]), _other(rng, k14[2], k14[3])
    batches["classes14"] = dict(queries=both([k14[:3] + s1 + k14[4:10] + s2 + k14[11:],             # two substitutions
                                              k14[:3] + s1 + k14[4:9] + x1 + k14[9:],               # a substitution and an insertion
                                              k14[:3] + x2 + k14[3:6] + "C" + k14[6:],              # two insertions, one in the CC run
                                              "G" + k14 + "T",                                      # one in front, one behind
                                              "G" + k14[:10] + s2 + k14[11:]]),                     # one in front and a substitution
                                kw=dict(distance=2, max_locations=5000, max_neighborhood=100000), family="k14")

    # ---- ties
    runs = [("A", 5), ("AC", 4), ("ACG", 3), ("T", 4), ("GT", 3), ("TTG", 2), ("C", 6), ("AT", 5), ("CAG", 3), ("G", 7), ("CT", 4), ("GAT", 4),
            ("A", 4), ("TC", 3), ("AAG", 3), ("T", 6), ("GA", 5), ("CCA", 2)]
    lens = [12, 13, 14, 16, 18, 20, 21, 24, 25, 27, 30, 32, 15, 19, 22, 28, 31, 32]
    tq = []
    batches["ties"] = dict(queries=tq, kw=dict(distance=1), runs=[])
    for qi, ((unit, reps), n) in enumerate(zip(runs, lens)):
        run = unit * reps
        rest = n - len(run)
        nl = [0, rest // 2, rest][qi % 3]            # the run opens the query, sits inside it, closes it
        left, right = _rand(rng, nl), _rand(rng, rest - nl)
        if left:
            left = left[:-1] + _other(rng, unit[-1], unit[0])
        if right:
            right = _other(rng, unit[0], unit[-1]) + right[1:]
        q = left + run + right
        rs, re = nl, nl + len(run)
        fw = qi % 2 == 0
        tq.append(q if fw else revcomp(q))
        batches["ties"]["runs"].append((rs, re))
        places = {"first": 0, "last": n - 1, "inside": rs + len(run) // 2, "edge": rs if rs > 0 else re - 1}
        for place, i in places.items():
            for kind in ("sub", "del", "ins"):
                if kind == "sub":
                    s = q[:i] + _other(rng, q[i]) + q[i + 1:]
                elif kind == "del":
                    s = q[:i] + q[i + 1:]
                elif place == "first":
                    s = q[0] + _other(rng, q[0], q[1]) + q[1:]
                elif place == "last":
                    s = q[:-1] + _other(rng, q[-1], q[-2]) + q[-1:]
                else:
                    s = q[:i] + q[i] + q[i:]         # the run grows by one character: the gap can sit anywhere in it
                if q in s:       # a run that opens or closes the query grew by one character: the query itself is still there
                    continue
                # flanks that continue the run where the query begins or ends with it, unless the window then holds the query itself
                pre = (unit[-1] if rs == 0 else _other(rng, q[0])) + ""
                post = unit[0] if re == n else _other(rng, q[-1])
                pre, post = _rand(rng, 1) + pre, post + _rand(rng, 1)
                if q in pre + s + post:
                    pre, post = pre[0] + _other(rng, q[0], pre[1]), _other(rng, q[-1], post[0]) + post[1]
                assert q not in pre + s + post
                plant_case("ties", qi, kind, place, fw, s, pre, post, 1, 1)

    # ---- clean
    bg = "".join(seqs[0])
    cl = []
    while len(cl) < 160:
        a = rng.randrange(4000, len(bg) - 1200)
        q = bg[a:a + 20]
        if len(cl) % 3 == 2:
            k = rng.randrange(2, 18)
            q = q[:k] + _other(rng, q[k]) + q[k + 1:]
        cl.append(q if len(cl) % 4 else revcomp(q))
    batches["clean"] = dict(queries=cl, kw=dict(distance=1))
    batches["clean_d2"] = dict(queries=cl[:48], kw=dict(distance=2, max_neighborhood=100000))

    # ---- lengths and deep: every planted string is taken from the query's own neighbourhood as the reference enumerates it
    def from_neighbourhood(batch, lengths, distance, cap, ci):
        qs = []
        for n in lengths:      # (three different letters at either end: the tie cases below need that, on either strand)
            q = _rand(rng, n)
            qs.append("".join(rng.sample("ACGT", 3)) + q[3:-3] + "".join(rng.sample("ACGT", 3)))
        kw = dict(distance=distance, max_neighborhood=cap, max_locations=20000)
        batches[batch] = dict(queries=qs, kw=kw, maxlen=max(lengths), literal=cap == NBHD_SMALL)
        for qi, q in enumerate(qs):
            fw = qi % 2 == 0
            qq = q if fw else revcomp(q)
            nb = O.neighbors(qq, distance, True, cap) if cap == NBHD_SMALL else O.neighbors_fast(qq, distance, True, cap)
            top = max(len(s) for s in nb)
            for kind, want in (("del", top - 2 if top > len(q) else top - 1), ("sub", top - 1 if top > len(q) else top), ("ins", top)):
                pool = [s for s in nb if len(s) == want] or [s for s in nb if len(s) >= len(q) - 1] or list(nb)
                s = pool[rng.randrange(len(pool))]
                plant_case(batch, qi, kind, "any", fw, s, _rand(rng, distance), _rand(rng, distance), ci, distance)
            # From distance 2 on a horizontal and a vertical move can tie on an optimal path.  The reference's walk begins with the
            # deletions of the first characters, so q[2:] and q[3:] are kept strings under any cap.  Planted are q[1] x q[2:] and
            # q[0] x q[1] q[3:], x the letter that q[0], q[1], q[2] leave: a gap in the query row and one in the window row, a
            # match between them, against two mismatches, all of cost 2; needle.h:105-131 picks horizontal, then vertical, then
            # diagonal
            if distance >= 2:
                x = _other(rng, qq[0], qq[1], qq[2])
                for s in (qq[1] + x + qq[2:], qq[0] + x + qq[1] + qq[3:]):
                    plant_case(batch, qi, "tie", "first", fw, s, _rand(rng, distance), _rand(rng, distance), ci, distance)
        # and one string of the first query's Hamming neighbourhood, for the batch's forward-only Hamming variant
        if not batch.startswith("len"):
            return
        pool = [s for s in O.neighbors(qs[0], distance, False, cap) if s != qs[0]]
        plant_case(batch, 0, "ham", "any", True, pool[rng.randrange(len(pool))], _rand(rng, distance), _rand(rng, distance), ci, distance)
    e1, e2 = cells_edge(1), cells_edge(2)
    for n in (24, 25, 32):
        from_neighbourhood("len%d_d3" % n, [n, n - 3, n - 7], 3, NBHD_SMALL, 2)
        from_neighbourhood("len%d_d1" % n, [n, n - 3, n - 7], 1, 10000, 2)
    for n in (33,) + e1 + (MAX_QLEN, MAX_QLEN + 1, 300):
        from_neighbourhood("len%d_d1" % n, [n, n - 3, n - 7], 1, 10000, 2)
    for n in e2:
        from_neighbourhood("len%d_d2" % n, [n, n - 3, n - 7], 2, NBHD_SMALL, 2)
    for n in (MAX_QLEN, MAX_QLEN + 1, 300):
        from_neighbourhood("len%d_d2" % n, [n, n - 7], 2, NBHD_SMALL, 1)
    from_neighbourhood("deep3", [12, 13, 14, 15], 3, NBHD_SMALL, 0)
    from_neighbourhood("deep4", [14, 15, 14, 15], 4, NBHD_SMALL, 0)
    for name in [b for b in batches if b.startswith("len")]:
        b = batches[name]
        batches[name + "_ham"] = dict(queries=b["queries"], kw=dict(b["kw"], hamming=True, forward_only=True), maxlen=b["maxlen"],
                                      literal=b["literal"], variant_of=name)

    # ---- each family at the other distance too: the band of 13 diagonals on the 20-nt family, the band of 7 on the 14-nt family
    s3, s4 = _other(rng, k20[4]), _other(rng, k20[15])
    batches["classes20_d2"] = dict(queries=both(["A" + k20 + "T", k20[:4] + s3 + k20[5:15] + s4 + k20[16:]]),
                                   kw=dict(distance=2, max_locations=5000, max_neighborhood=100000), family="k20")
    batches["classes14_d1"] = dict(queries=both(["G" + k14, k14 + "T", k14[:6] + "C" + k14[6:]]),
                                   kw=dict(distance=1, max_locations=5000), family="k14")
    for name in CLASS_BATCHES:     # the family's string is a kept string of every query: in its neighbourhood and substring-minimal
        b = batches[name]
        for q in b["queries"][::2]:
            assert fam[b["family"]]["string"] in O.neighbors_fast(q, b["kw"]["distance"], True, 100000), (name, q)

    seqs = ["".join(s) for s in seqs]
    text = ("\n".join(seqs) + "\n").encode()
    assert len(text) <= 250000
    g = {"seqs": seqs, "names": NAMES, "text": text, "seqlen": [len(x) + 1 for x in seqs], "batches": batches, "plants": plants,
         "families": fam, "regions": regions}
    _check_unique(g)
    _memo["g"] = g
    return g


def _check_unique(g):
    """a planted string occurs in the text where a planted region holds it and nowhere in the background; a family's string occurs
    once per copy"""
    seen = {}
    for p in g["plants"]:
        seen.setdefault(p["planted"], p)
    for s, p in seen.items():
        if len(s) < 12:      # (distance 3 / 4 keeps strings of 8-11 nt: those occur by chance, and the checker finds them too)
            continue
        inside = sum(_overlapping(r, s) for _, _, r in g["regions"])
        found = len(O.bf_locate(g["text"], s.encode()))
        assert found == inside and found >= 1, (p["batch"], p["query"], p["kind"], p["place"], s, found, inside)
    for name, f in g["families"].items():
        want = len(f["at"])
        assert len(O.bf_locate(g["text"], f["string"].encode())) == want == len(set(f["at"])), (name, want)


def batches():
    return genome()["batches"]


LENGTH_BATCHES = (["len%d_d3" % n for n in (24, 25, 32)] + ["len%d_d1" % n for n in (24, 25, 32, 33) + cells_edge(1) + (255, 256, 300)] +
                  ["len%d_d2" % n for n in cells_edge(2) + (255, 256, 300)])
DEEP_BATCHES = ["deep3", "deep4"]
BATCH_NAMES = ["ties", "clean", "clean_d2"] + CLASS_BATCHES + LENGTH_BATCHES + [n + "_ham" for n in LENGTH_BATCHES] + DEEP_BATCHES


def oracle_index():
    """the oracle's index of the text, written once per process: (Index, path of the .fm9 file)"""
    if "ix" not in _memo:
        g = genome()
        import atexit
        import shutil
        d = tempfile.mkdtemp(prefix="verify_shapes_")
        atexit.register(shutil.rmtree, d, True)
        path = os.path.join(d, "verify.fm9")
        O.build_fm9(g["text"], path)
        _memo["ix"] = (O.Index(path), path)
    return _memo["ix"]


def expected(name):
    """the oracle's hits of a batch in push order: [(query, score, chr, start, strand, refalign, queryalign)]"""
    key = ("hits", name)
    if key not in _memo:
        g = genome()
        b = g["batches"][name]
        O.fast_neighbors(not b.get("literal"))
        try:
            _, hits = oracle_index()[0].hunt(g["seqlen"], g["names"], b["queries"], want_hits=True, **b["kw"])
        finally:
            O.fast_neighbors(False)
        _memo[key] = hits
    return _memo[key]


def context(text, loc, m, d):
    """hunter.h:363-382 for a kept string of m characters at text position loc: (pre_eff, post_eff, the context's bytes)"""
    n = len(text) + 1            # the index text ends in the sentinel
    pre, post = min(d, loc), d
    if loc + m + post > n:
        post = n - loc - m
    left = text[loc - pre:loc].decode("latin-1")
    right = text[loc + m:loc + m + post].decode("latin-1")
    if "\n" in left:
        left = left[left.rfind("\n") + 1:]
    if "\n" in right:
        right = right[:right.find("\n")]
    return len(left), len(right), left + "|" + right


def push_list(name):
    """the loop of hunter.h:489-543 over the batch, in Python: one dict per pushed hit, in push order, with what the oracle's list does
    not say: the text position, the kept string that was located there, the position inside its sequence and the hit's class"""
    key = ("push", name)
    if key in _memo:
        return _memo[key]
    g = genome()
    b = g["batches"][name]
    kw = b["kw"]
    d0, indel, cap = kw["distance"], not kw.get("hamming"), kw.get("max_neighborhood", 10000)
    maxloc = kw.get("max_locations", 1000)
    orc = oracle_index()[0]
    starts = [0]
    for n in g["seqlen"]:
        starts.append(starts[-1] + n)
    nb_of = O.neighbors if b.get("literal") else O.neighbors_fast
    out = []
    for qi, q in enumerate(b["queries"]):
        d = min(d0, len(q) - 1)
        hits = 0
        for strand, qq in (("+", q), ("-", revcomp(q))):
            if strand == "-" and kw.get("forward_only"):
                break
            for s in nb_of(qq, d, indel, cap):
                if hits >= maxloc:
                    break
                locs = sorted(orc.locate(s.encode()))
                for loc in locs[:maxloc]:
                    if hits >= maxloc:
                        break
                    ref = max(i for i in range(len(g["seqlen"])) if starts[i] <= loc)
                    pe, po, ctx = context(g["text"], loc, len(s), d if indel else 0)
                    out.append(dict(query=qi, strand=strand, kept=s, loc=loc, chr=ref, chrpos=loc - starts[ref],
                                    cls=(s, pe, po, ctx)))
                    hits += 1
    exp = expected(name)
    assert len(out) == len(exp), (name, len(out), len(exp))
    for k, (a, e) in enumerate(zip(out, exp)):
        assert (a["query"], a["chr"], a["strand"]) == (e[0], e[2], e[4]), (name, k, a, e)
    _memo[key] = out
    return out


def window_of(name, hit):
    """the window needle() sees for a pushed hit, and the query's strand as it is aligned"""
    g = genome()
    q = g["batches"][name]["queries"][hit["query"]]
    s, pe, po, _ = hit["cls"]
    return g["text"][hit["loc"] - pe:hit["loc"] + len(s) + po].decode("latin-1"), (q if hit["strand"] == "+" else revcomp(q))


def planted_hits(name):
    """for every planted case of a batch: (case, [indices into the push list of this query's hits that lie on the planted string])"""
    pl = push_list(name)
    g = genome()
    base = name[:-4] if name.endswith("_ham") else name
    starts = [0]
    for n in g["seqlen"]:
        starts.append(starts[-1] + n)
    out = []
    for p in g["plants"]:
        if p["batch"] != base:
            continue
        lo = starts[p["seq"]] + p["at"]
        hi = lo + len(p["planted"])
        out.append((p, [k for k, h in enumerate(pl) if h["query"] == p["query"] and h["strand"] == p["strand"] and
                        lo - 1 <= h["loc"] and h["loc"] + len(h["kept"]) <= hi + 1]))
    return out
