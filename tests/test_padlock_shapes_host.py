"""tests/padlock_shapes.py without a GPU: the model runs every matrix entry over the reference's own thal() (oracle/_ref) and the
oracle's count() / neighbors(), and the inputs must reach what they were built for, counted on the reference side alone.  These are
the conditions that make tests/test_gpu_padlock_shapes.py meaningful: a genome, an exon list or a parameter set that quietly
stopped producing its case fails here, not there."""
import pytest

import oracle_lib as O
import padlock_shapes as P
import thal_expect as TE

needs_ref = pytest.mark.skipif(not TE.have_ref(), reason="oracle/_ref (the reference's thal.h built in place) is not available")


def test_genome_holds_its_planted_features():
    g = P.genome()
    a, b, c = g["seqs"]
    text = g["text"].decode()
    assert 60000 <= len(text) <= 100000 and text == text.upper() and set(text) <= set("ACGTNRY\n")
    src, dst, n = P.DUP
    assert a[src:src + n] == b[dst:dst + n] and text.count(a[src + 100:src + 140]) == 2
    src, dst, n = P.NEAR
    diff = [k for k in range(n) if a[src + k] != b[dst + k]]
    assert diff == list(range(10, n, 37))
    src, dst, n = P.RC
    assert c[dst:dst + n] == P.revcomp(a[src:src + n]) and text.count(a[src + 100:src + 140]) == 1
    assert a[P.N_RUN[0]:P.N_RUN[0] + P.N_RUN[1]] == "N" * P.N_RUN[1] and text.count("N") == P.N_RUN[1]
    assert (b[P.R_AT], b[P.Y_AT]) == ("R", "Y") and text.count("R") == text.count("Y") == 1
    assert P.IUPAC_EXON[0] < P.R_AT < P.Y_AT < P.IUPAC_EXON[1]
    assert P.revcomp("ACGTURYSWKMBVDHNX") == "NNDHBVKMWSRYAACGT"


@pytest.mark.parametrize("armlen", sorted({p[0] for p in P.MATRIX}))
def test_exon_list_holds_its_cases(armlen):
    g = P.genome()
    text = g["text"].decode()
    L, T = armlen, 2 * armlen
    ex = dict(P.named_exons(armlen))
    names = [n for n, _ in P.named_exons(armlen)]
    assert len(ex) == len(names)
    lens = {n: len(s) for n, s in ex.items()}
    assert (lens["two_arms"], lens["short"], lens["empty"], lens["two_arms_plus_1"]) == (T, T - 1, 0, T + 1)
    assert names[0] == "two_arms" and names[-1] == "two_arms_plus_1" and names.index("empty") == names.index("short") + 1
    assert 0 < names.index("short") < len(names) - 2
    in_text = lambda s: s in text
    for n in ("dup", "near", "rc_copy", "n_inside", "n_last", "iupac", "identical_1", "overlap_1", "overlap_2", "two_arms", "short"):
        assert in_text(ex[n]), n
    assert not in_text(ex["minus_strand"]) and in_text(P.revcomp(ex["minus_strand"]))
    assert text.count(ex["dup"][100:140]) == 2 and in_text(P.revcomp(ex["rc_copy"][100:140]))
    assert not any(in_text(ex["foreign"][k:k + 16]) or in_text(P.revcomp(ex["foreign"][k:k + 16])) for k in range(0, 284, 4))
    n_in = ex["n_inside"]
    assert "N" in n_in and n_in.find("N") >= T and len(n_in) - n_in.rfind("N") - 1 >= T       # probes on both sides of the run
    assert ex["n_last"].count("N") == 1 and ex["n_last"][-1] == "N" and lens["n_last"] >= T
    assert ex["iupac"].count("R") == ex["iupac"].count("Y") == 1
    assert ex["identical_1"] == ex["identical_2"] and names.index("identical_2") - names.index("identical_1") > 1
    assert ex["overlap_1"][-100:] == ex["overlap_2"][:100]
    assert ex["near_piece"] in ex["near"]
    for p in P.MATRIX:
        if p[0] == armlen:       # the capped lists keep every length around 2L, first, adjacent in the middle and last
            sub = P.exons(p)
            assert len(sub[0]) == T and len(sub[-1]) == T + 1 and any((len(x), len(y)) == (T - 1, 0) for x, y in zip(sub, sub[1:]))
            assert 100 <= sum(len(s) - L + 1 for s in sub if len(s) >= T) <= 5000


def test_matrix_covers_what_the_scan_branches_on():
    M = P.MATRIX
    assert len(set(M)) == len(M) and {p[0] for p in M} >= {10, 15, 20, 24, 25}
    kinds = {(p[1], p[2]) for p in M}
    assert kinds >= {(0, False), (1, False), (1, True), (2, True), (2, False)}
    assert all(p[0] <= 20 for p in M if p[1] == 2 and not p[2])
    assert (20, 1, False, 2, 0.4, 0.6) in M and any(p[3:] == (10, 0.3, 0.7) for p in M)
    for L in (24, 25):     # both probe paths (paired on the device up to 48 nt, dg_thal_batch above) meet a neighbourhood count
        assert any(p[0] == L and p[1] > 0 for p in M)
    L, k = P.BOUNDARY[0], round(P.BOUNDARY[4] * P.BOUNDARY[0])
    assert k / L == P.BOUNDARY[4] and (L - k) / L == P.BOUNDARY[5] and P.BOUNDARY in M


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{params: (exons, model)} for the whole matrix, computed once"""
    fm9 = str(tmp_path_factory.mktemp("padlock_shapes") / "g.fm9")
    O.build_fm9(P.genome()["text"], fm9)
    orc = O.Index(fm9)
    memo = P.oracle_memo(orc, P.ref_thal_pairs)
    out = {p: (P.exons(p), memo.model(P.exons(p), p)) for p in P.MATRIX}
    out["count"] = lambda s: orc.count(s.encode())
    return out


def _slots(exons, m, L):
    """(slot, exon number, q, exon) of every arm slot"""
    for e, ex in enumerate(exons):
        for q in range(m["pos_off"][e + 1] - m["pos_off"][e]):
            yield m["pos_off"][e] + q, e, q, ex


def _facts(params, exons, m):
    L, distance, hamming, tmdiff, gc_min, gc_max = params
    T = 2 * L
    passes = lambda g: not (g < gc_min or g > gc_max)
    over = lambda at: m["arm_tm"][at] > 93 + m["arm_gc"][at] - 675.0 / L
    f = dict(in_window=set(), outside=0, tmdiff_alone=0, ceiling_alone=0, both_sides=0, first_degree=0, last_degree=0, counted=[])
    for at, e, q, ex in _slots(exons, m, L):
        if m["arm_count"][at] >= 0:
            f["counted"].append((at, ex[q:q + L]))
        if q + T > len(ex):
            continue
        if m["probe_tm"][at] != P.NOT_COMPUTED:
            if P.in_window(m["probe_tm"][at], m["probe_gc"][at], L):
                f["in_window"].add(at)
                f["both_sides"] += q >= L and at - L in f["in_window"]
                lo = 81.5 + m["probe_gc"][at] - 675.0 / T
                f["first_degree"] += m["probe_tm"][at] < lo + 1       # a window cut short at either end would lose these
                f["last_degree"] += m["probe_tm"][at] > lo + 9
            else:
                f["outside"] += 1
        elif passes(m["arm_gc"][at]) and passes(m["arm_gc"][at + L]) and passes(m["probe_gc"][at]):
            far = abs(m["arm_tm"][at] - m["arm_tm"][at + L]) > tmdiff
            hot = over(at) or over(at + L)
            f["tmdiff_alone"] += far and not hot
            f["ceiling_alone"] += hot and not far
    return f


@needs_ref
@pytest.mark.parametrize("params", P.MATRIX, ids=P.entry_id)
def test_every_entry_counts_enough_arms(models, params):
    exons, m = models[params]
    f = _facts(params, exons, m)
    print("%s: %d positions, %d arm thal, %d probe thal, %d probes inside the window, %d outside, %d arms counted, %d arms on both "
          "sides, refused by tmdiff alone %d, by the ceiling alone %d" %
          (P.entry_id(params), m["pos_off"][-1], m["n_arm_thal"], m["n_probe_thal"], len(f["in_window"]), f["outside"],
           m["n_arms_counted"], f["both_sides"], f["tmdiff_alone"], f["ceiling_alone"]))
    edit2 = params[1] == 2 and not params[2]
    assert m["n_arms_counted"] >= (10 if edit2 else 100)
    assert m["n_arms_counted"] == len(f["counted"]) == len({a for at in f["in_window"] for a in (at, at + params[0])})
    assert m["n_arm_thal"] >= m["n_probe_thal"] >= len(f["in_window"]) > 0
    assert -2 not in m["arm_count"] and -2 not in m["arm_nbcount"]
    if params[1] == 0:
        assert set(m["arm_nbcount"]) == {-1}
    else:
        assert all((n >= c >= 0) or (n == c == -1) for n, c in zip(m["arm_nbcount"], m["arm_count"]))   # an arm is its own neighbour


@needs_ref
def test_the_matrix_reaches_every_count_case(models):
    seen = dict(twice=0, zero=0, neighbours=0, reverse=0, iupac=0, both_sides=0, outside=0, tmdiff_alone=0, ceiling_alone=0,
                first_degree=0, last_degree=0)
    for params in P.MATRIX:
        exons, m = models[params]
        f = _facts(params, exons, m)
        for k in ("both_sides", "outside", "tmdiff_alone", "ceiling_alone", "first_degree", "last_degree"):
            seen[k] += f[k]
        for at, arm in f["counted"]:
            c, nb = m["arm_count"][at], m["arm_nbcount"][at]
            seen["twice"] += c >= 2
            seen["zero"] += c == 0
            seen["neighbours"] += nb > c
            seen["iupac"] += "R" in arm or "Y" in arm
            seen["reverse"] += models["count"](P.revcomp(arm)) > 0
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


@needs_ref
def test_the_boundary_entry_sits_on_both_gc_bounds(models):
    """gc_min = 9/20 and gc_max = 11/20: arms and probes exactly on a bound pass (`<` and `>`, padlock.h:331), the next value fails"""
    L, _, _, _, gc_min, gc_max = P.BOUNDARY
    exons, m = models[P.BOUNDARY]
    k_lo, k_hi = round(gc_min * L), round(gc_max * L)
    at_value = lambda k: [at for at in range(m["pos_off"][-1]) if m["arm_gc"][at] == k / L]
    for k, passes in ((k_lo, True), (k_lo - 1, False), (k_hi, True), (k_hi + 1, False)):
        slots = at_value(k)
        assert slots, k
        assert all((m["arm_tm"][at] != P.NOT_COMPUTED) == passes for at in slots), k
    on = [at for at in range(m["pos_off"][-1]) if m["probe_tm"][at] != P.NOT_COMPUTED and m["probe_gc"][at] in (gc_min, gc_max)]
    assert on
