"""tests/verify_shapes.py without a GPU: the oracle runs every batch, and each batch must still have the property it was built for,
counted on the reference side alone (the oracle's hit list, the push list rebuilt from the text, a plain Needleman-Wunsch below).  A
generator that quietly stopped producing its shape fails here, not in the GPU module."""
import pytest

import oracle_lib as O
import verify_shapes as V


def optimal_paths(window, query):
    """(score, number of optimal tracebacks) of needle() as hunt calls it: rows = window, columns = query, match 0, mismatch and gaps
    -1, moves down column 0 and down the last column free.  Every move that reaches a cell's maximum counts."""
    m, n = len(window), len(query)
    sc = [[0] * (n + 1) for _ in range(m + 1)]
    cnt = [[1] * (n + 1) for _ in range(m + 1)]     # row 0: horizontal moves only; column 0: vertical moves only
    for c in range(n + 1):
        sc[0][c] = -c
    for r in range(1, m + 1):
        for c in range(1, n + 1):
            d = sc[r - 1][c - 1] - (window[r - 1] != query[c - 1])
            v = sc[r - 1][c] - (c != n)
            h = sc[r][c - 1] - 1
            best = max(d, v, h)
            sc[r][c] = best
            cnt[r][c] = (cnt[r - 1][c - 1] if d == best else 0) + (cnt[r - 1][c] if v == best else 0) + (cnt[r][c - 1] if h == best else 0)
    return sc[m][n], cnt[m][n]


def _wanted(name, p):
    """the planted cases a batch answers for: the Hamming variants find the string planted for them, on the forward strand"""
    return (p["kind"] == "ham") == name.endswith("_ham")


@pytest.mark.parametrize("name", V.BATCH_NAMES)
def test_every_planted_copy_is_reported_with_its_score(name):
    """no planted case without a hit, and a hit on it carries the score a plain Needleman-Wunsch (verify_shapes.nw_score) gives the
    query against the planted string and its flanks; every hit's score lies in -distance..0 and is that of its own window"""
    exp, pl = V.expected(name), V.push_list(name)
    kw = V.batches()[name]["kw"]
    cases = [(p, idx) for p, idx in V.planted_hits(name) if _wanted(name, p)]
    missing = [(p["query"], p["kind"], p["place"]) for p, idx in cases if not idx]
    wrong = [(p["query"], p["kind"], p["place"], p["score"], [exp[k][1] for k in idx]) for p, idx in cases
             if idx and p["score"] not in [exp[k][1] for k in idx]]
    print("%s: %d queries, %d hits, %d planted cases, %d without a hit" % (name, len(V.batches()[name]["queries"]), len(exp), len(cases),
                                                                         len(missing)))
    assert not missing and not wrong, (name, missing, wrong)
    if name not in ["clean", "clean_d2"] + V.CLASS_BATCHES:      # (the families are counted copy by copy below)
        assert cases
    hit_queries = {e[0] for e in exp}
    if name in V.CLASS_BATCHES + ["ties"] + V.LENGTH_BATCHES + V.DEEP_BATCHES:
        assert hit_queries == set(range(len(V.batches()[name]["queries"]))), (name, sorted(hit_queries))
    step = max(1, len(exp) // 300)
    for k in range(0, len(exp), step):
        w, q = V.window_of(name, pl[k])
        if kw.get("hamming"):
            want = -sum(1 for a, b in zip(w, q) if a != b)
        else:
            want = V.nw_score(w, q)
        assert exp[k][1] == want and -kw["distance"] <= want <= 0, (name, k, pl[k], exp[k])


def test_ties_have_more_than_one_optimal_alignment():
    """every planted case of `ties` has score -1; all but the substitutions strictly inside the query have two or more optimal
    tracebacks (a substitution there has no second path of cost 1 through it: the control group); at least 30 hits drop leading query-gap columns"""
    exp, pl = V.expected("ties"), V.push_list("ties")
    qs = V.batches()["ties"]["queries"]
    tied = single = controls = lead_pos = 0
    kinds = set()
    for p, idx in V.planted_hits("ties"):
        assert p["score"] == -1, p
        # controls: a substitution strictly inside the query, and a deletion between two other characters (inside a 2- or 3-nt unit):
        # no second path of cost 1 leads through such an edit.  Every other case ties: the first and the last column (gap or
        # mismatch), an inserted character beside its equal, a deleted character beside its equal
        i0 = _edit_index(p, qs)
        qq = qs[p["query"]] if p["strand"] == "+" else V.revcomp(qs[p["query"]])
        slides = p["kind"] == "ins" or (p["kind"] == "del" and i0 > 0 and qq[i0] == qq[i0 - 1])
        interior_sub = p["place"] in ("inside", "edge") and 0 < i0 < len(qq) - 1 and not slides
        best = 0
        for k in idx:
            w, q = V.window_of("ties", pl[k])
            score, paths = optimal_paths(w, q)
            assert score == exp[k][1] == -1, (p, k)
            best = max(best, paths)
            sc, ra, qa, lead = O.needle_hunt(w, q)
            assert (sc, ra, qa) == (exp[k][1], exp[k][5], exp[k][6])
            lead_pos += lead > 0
        if interior_sub:
            controls += 1
            single += best == 1      # (a tie here can only come from the window's ends: no other path through the edit costs 1)
        else:
            assert best >= 2, (p, best)
            tied += 1
            kinds.add((p["kind"], p["place"], p["strand"]))
    print("ties: %d cases with two or more optimal alignments, %d controls with one only, %d hits with lead > 0" %
          (tied, single, lead_pos))
    assert (tied, controls, single, lead_pos) == TIES_SPLIT, (tied, controls, single, lead_pos)
    assert {(k, pl_) for k, pl_, _ in kinds} >= {(k, pl_) for k in ("del", "ins") for pl_ in ("first", "last", "inside", "edge")} | \
        {("sub", "first"), ("sub", "last")}
    assert {s for _, _, s in kinds} == {"+", "-"}


# what the seeded generator produces: cases asserted to tie, controls, controls with exactly one optimal traceback, hits with lead > 0
TIES_SPLIT = (150, 54, 42, 191)


def _edit_index(p, qs):
    """where the planted string first differs from the query's own strand"""
    q = qs[p["query"]] if p["strand"] == "+" else V.revcomp(qs[p["query"]])
    return next((i for i, (a, b) in enumerate(zip(p["planted"], q)) if a != b), len(q) - 1)


@pytest.mark.parametrize("name,dist,nfam,edges", [("classes20", 1, V.F20_BULK + 5, (1024, 2048)), ("classes14", 2, V.F14_BULK + 5, (1024, 2048)),
                                                  ("classes20_d2", 2, V.F20_BULK + 5, (1024,)), ("classes14_d1", 1, V.F14_BULK + 5, (1024,))])
def test_classes_share_a_string_and_differ_in_their_answers(name, dist, nfam, edges):
    g = V.genome()
    exp, pl = V.expected(name), V.push_list(name)
    b = g["batches"][name]
    k = g["families"][b["family"]]["string"]
    fam = [i for i, h in enumerate(pl) if h["kept"] in (k, V.revcomp(k))]
    per_query = [sum(1 for i in fam if pl[i]["query"] == q) for q in range(len(b["queries"]))]
    assert per_query == [nfam] * len(b["queries"]), per_query      # no copy is cut, none is missed
    assert nfam >= 192 and nfam < b["kw"]["max_locations"]
    fwd = [i for i in fam if pl[i]["query"] == 0]
    tuples = {pl[i]["cls"][1:] for i in fwd}
    ctx = {pl[i]["cls"][3] for i in fwd}
    # the query that inserts a character in front of the string (query 0 at distance 1, query 6 at distance 2): the flank decides
    flank_q = [i for i in fam if pl[i]["query"] == (6 if name == "classes14" else 0)]
    answers = {(exp[i][5], exp[i][6]) for i in flank_q}
    shifts = {exp[i][3] - 1 - pl[i]["chrpos"] for i in flank_q}
    scores = {exp[i][1] for i in flank_q}
    print("%s: %d hits, %d of the family; query 0: %d classes, %d alignments, start - position in %s, scores %s" %
          (name, len(pl), len(fam), len(tuples), len(answers), sorted(shifts), sorted(scores)))
    # all 16 A/C/G/T pairs next to the string; N, R, Y on either side; the four sequence-edge placements and the two ends of the text
    inner = {(c.split("|")[0][-1:], c.split("|")[1][:1]) for c in ctx}
    assert inner >= {(a, c) for a in "ACGT" for c in "ACGT"}
    for x in "NRY":
        assert any(a == x for a, _ in inner) and any(c == x for _, c in inner), x
    assert {(t[0], t[1]) for t in tuples} >= {(dist, dist), (0, dist), (dist, 0)}
    if dist == 2:
        assert {(t[0], t[1]) for t in tuples} >= {(1, 2), (2, 1)}
    assert len(tuples) >= 16 + 6 + 2      # A/C/G/T pairs, N / R / Y either side, nothing in front, nothing behind
    assert len(answers) >= 2 and len(shifts) >= 2 and len(scores) >= 2
    # the first position of the text and the last one before the final separator
    locs = {pl[i]["loc"] for i in fam}
    if b["family"] == "k20":
        assert 0 in locs
    else:
        assert len(g["text"]) - 1 - len(k) in locs
    # a separator right in front of a copy that is not at text position 0 (the cut at '\n', not the clamp at the text's start), and
    # right behind a copy that does not end the text; at distance 2 also a separator two characters away on either side
    assert any(pl[i]["cls"][1] == 0 and pl[i]["loc"] > 0 for i in fam)
    assert any(pl[i]["cls"][2] == 0 and pl[i]["loc"] + len(k) < len(g["text"]) - 1 for i in fam)
    if dist == 2:
        assert any(pl[i]["cls"][1] == 1 and pl[i]["loc"] > 1 for i in fam) and any(pl[i]["cls"][2] == 1 for i in fam)
    # hunter.h:382 compares with <: a string at offset pre_eff of its sequence keeps its position
    quirk = [i for i in fam if pl[i]["cls"][1] == pl[i]["chrpos"] > 0]
    assert quirk and all(exp[i][3] - 1 >= pl[i]["chrpos"] for i in quirk)
    # the family's hits lie on both sides of hit 1 024 and of hit 2 048 of the batch: two workgroups of 256 * 4 and of 256 * 8 hits
    for edge in edges:
        assert edge - 1 in fam and edge in fam, edge
    # hits that bring their context along (A/C/G/T on all sides) next to hits that read the text
    plain = [i for i in fam if set(pl[i]["cls"][3]) <= set("ACGT|") and pl[i]["cls"][1:3] == (dist, dist)]
    assert plain and len(plain) < len(fam)


@pytest.mark.parametrize("name", V.LENGTH_BATCHES + [n + "_ham" for n in V.LENGTH_BATCHES])
def test_length_batches_have_the_named_longest_query(name):
    b = V.batches()[name]
    n = int(name[3:].split("_")[0])
    assert max(len(q) for q in b["queries"]) == n == b["maxlen"] and len(b["queries"]) <= 4
    assert len(V.expected(name)) >= 1


def test_length_batches_cover_every_boundary_of_the_dispatch():
    """hunt.hip run_batch: maxlen <= 24, <= 32, cells <= 32 * 160, MAX_QLEN; the band takes maxlen <= 32 at distance <= 2"""
    for d in (1, 2):
        lo, hi = V.cells_edge(d)
        assert V.cells(lo, d) <= V.FULL_MATRIX_CELLS < V.cells(hi, d) and hi == lo + 1
        assert "len%d_d%d" % (lo, d) in V.LENGTH_BATCHES and "len%d_d%d" % (hi, d) in V.LENGTH_BATCHES
    for n in (24, 25, 32):
        assert "len%d_d3" % n in V.LENGTH_BATCHES and "len%d_d1" % n in V.LENGTH_BATCHES
    for n in (33, 255, 256, 300):
        assert "len%d_d1" % n in V.LENGTH_BATCHES


@pytest.mark.parametrize("name,dist", [("deep3", 3), ("deep4", 4)])
def test_deep_batches_drop_leading_columns(name, dist):
    """queries of 12-15 nt at distance 3 and 4: hits whose alignment drops `dist` leading query-gap columns, and hits with an edit"""
    exp, pl = V.expected(name), V.push_list(name)
    qs = V.batches()[name]["queries"]
    assert all(12 <= len(q) <= 15 for q in qs)
    leads = {}
    for k in range(len(exp)):
        w, q = V.window_of(name, pl[k])
        sc, ra, qa, lead = O.needle_hunt(w, q)
        assert (sc, ra, qa) == (exp[k][1], exp[k][5], exp[k][6]), (name, k)
        leads[lead] = leads.get(lead, 0) + 1
    print("%s: %d hits, leading columns dropped %s, scores %s" % (name, len(exp), sorted(leads.items()), sorted({e[1] for e in exp})))
    assert leads.get(dist, 0) >= 3 and leads.get(dist - 1, 0) >= 1
    assert min(e[1] for e in exp) == -dist


def test_the_schedules_reach_the_widths_they_name():
    """run_batch sizes the hit buffer from the handle's history (hit_cap = max(hint, 4 nq + 1024), hint = nhits * 5 / 4 + 1024 of the
    largest batch so far, a batch with more hits than room is repeated with that room) and picks k_verify_memo's hits per lane from
    hit_cap / nq: distance 1: >= 24 -> 4 (8 on a handle opened without the context records), >= 12 -> 4, else 1; distance 2:
    >= 192 -> 8, >= 96 -> 4, else 1.  The schedules of tests/test_gpu_verify_shapes.py, from the oracle's hit counts"""
    n = {name: len(V.expected(name)) for name in ("ties", "clean", "clean_d2", "classes20", "classes14")}
    nq = {name: len(V.batches()[name]["queries"]) for name in n}

    def room(hint, nhits, queries):
        cap = max(hint, 4 * queries + 1024)
        return cap if nhits <= cap else nhits + nhits // 4 + 1024
    # distance 1, fresh handle: ties + clean in one call -> 1
    cap = room(0, n["ties"] + n["clean"], nq["ties"] + nq["clean"])
    assert cap // (nq["ties"] + nq["clean"]) < 12
    # ties alone on a fresh handle -> 4 (8 without context records)
    assert room(0, n["ties"], nq["ties"]) // nq["ties"] >= 24
    # classes20 -> 4 / 8, and leaves a hint under which ties + clean run 4 hits per lane
    cap = room(0, n["classes20"], nq["classes20"])
    assert cap // nq["classes20"] >= 24
    hint = n["classes20"] + n["classes20"] // 4 + 1024
    both = n["classes20"] + n["ties"] + n["clean"]
    assert 12 <= room(hint, both, nq["classes20"] + nq["ties"] + nq["clean"]) // (nq["classes20"] + nq["ties"] + nq["clean"])
    # distance 2, fresh handle: clean_d2 -> 1; classes14 -> 8; classes14 + clean_d2 after it -> 4
    assert room(0, n["clean_d2"], nq["clean_d2"]) // nq["clean_d2"] < 96
    assert room(0, n["classes14"], nq["classes14"]) // nq["classes14"] >= 192
    hint = n["classes14"] + n["classes14"] // 4 + 1024
    q2 = nq["classes14"] + 20
    assert 96 <= room(hint, n["classes14"] + n["clean_d2"], q2) // q2 < 192


# ---- the tie order, kernel by kernel --------------------------------------------------------------------------------------------

rows_under = V.rows_under


TIE_MIN = 6      # two planted tie windows per query, three queries: what one batch of three queries at distance >= 2 must give


@pytest.mark.parametrize("kernel", ["k_verify<1,true,24>", "k_verify<1,true,32>", "k_verify<160,false>", "k_verify<2200,false>", "k_verify_long",
                                    "k_verify_memo<13>"])
def test_each_kernel_sees_hits_that_a_swapped_tie_order_changes(kernel):
    """over the batches that run on a kernel: the model above with needle.h's order gives the oracle's rows for every hit, and at least
    TIE_MIN hits change their rows when vertical is tried before horizontal, and when diagonal is tried first"""
    names = [n for n in V.LENGTH_BATCHES + V.DEEP_BATCHES if V.kernel_of(V.batches()[n]["maxlen"], V.batches()[n]["kw"]["distance"]) == kernel]
    if kernel == "k_verify_memo<13>":
        names = ["classes14", "classes20_d2"]
    assert names
    changed = {"vhd": 0, "dhv": 0}
    total = 0
    for name in names:
        exp, pl = V.expected(name), V.push_list(name)
        seen = {}
        for k in range(len(exp)):
            w, q = V.window_of(name, pl[k])
            if (w, q) not in seen:
                ref = rows_under(w, q, "hvd")
                seen[(w, q)] = (ref, {o: rows_under(w, q, o) != ref for o in changed})
            ref, diff = seen[(w, q)]
            assert ref[:2] == (exp[k][5], exp[k][6]) and exp[k][3] - 1 == pl[k]["chrpos"] - (pl[k]["cls"][1] if pl[k]["cls"][1] < pl[k]["chrpos"]
                                                                                            else 0) + ref[2], (name, k, pl[k], exp[k], ref)
            total += 1
            for o in changed:
                changed[o] += diff[o]
    print("%s: batches %s, %d hits, rows change under vertical-first for %d, under diagonal-first for %d" %
          (kernel, names, total, changed["vhd"], changed["dhv"]))
    assert changed["vhd"] >= TIE_MIN and changed["dhv"] >= TIE_MIN, (kernel, changed)
