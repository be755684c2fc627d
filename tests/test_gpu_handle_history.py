"""dg_hunt on the PRODUCT library, driven through its data-driven paths by what a handle ran before.

run_batch (dicey_amd/csrc/hunt.hip) keeps hints per handle: which kernel families the previous batches needed (generic kernels,
walker, short-string body of k_search2p, locate jobs; each sticky for STICKY batches), capacities that only grow, the LDS list size
of k_search1s, the hits per lane of k_verify_memo, the speculative classic fetch.  A batch that finds a hint wrong is repeated with
the other path.  A wrong hint may cost time, never hits: every answer here is compared with the checker (oracle_lib) on the hits in
push order and on each query's message vector, and HuntBatch.path shows that a schedule drove the path it claims.

No test switch is read here (conftest.EXP_VARS must be unset): the paths below are the ones the product reaches from data and
history.  Each switch of the development build maps to the product path that reaches the same kernels:

| forced switch          | data that reaches the same path on the product library          | observable                                 |
|------------------------|-----------------------------------------------------------------|--------------------------------------------|
| nofuse                 | a string above 42 characters at distance 1                      | flat_kernel_form 1                         |
| noband                 | queries of 33 nt or more, or distance above 2                    | verify_kernel_form 0                       |
| nofuse2 / nopre5d2     | a distance-2 batch with one query over 40 nt                    | flat_kernel_form 4 or 6                    |
| nolong2                | DICEY_KMER_K2=0, or the short-string schedule                    | flat_kernel_form 5                         |
| noprep                 | the generic-hint schedule                                       | flat_kernel_form 2                         |
| nodirectctx            | compact=True open, Hamming mode, distance 2                      | answers                                    |
| caps                   | the capacity schedule (hit, shard / flat and walker list retry) | nhits above the fresh hit capacity; answers |
| ch4 / ch8              | the verify-width schedule                                       | verify_kernel_form & 0xff 1, then 4 or 8   |
| lcap2                  | the LDS hand-over schedule (256 / 512 entries from history)      | form 3, then 2 (repeat), 3 on 512 entries  |
| caphost                | a capped batch that mixes device and host jobs                  | cap_queries_device and cap_queries_host > 0 |

Switches without a product path, not tested here: nonwin (DICEY_NO_N_WINDOW), noflatham2 (DICEY_NO_FLAT_HAMMING2), nominima
(DICEY_NO_SA_MINIMA; the product leaves the block minima out only on a device short of HBM)."""
import json
import os
import random

import pytest

import conftest
import dicey_amd
import oracle_lib as O
from conftest import genome_text, revcomp
from dicey_amd import _capi

pytestmark = pytest.mark.gpu

STICKY = 8  # batches a kernel-family hint stays on after the last batch that needed it (hunt.hip run_batch)
CHECK_THREADS = 16  # the checker's host threads (not os.cpu_count(): the GPU box shows the whole machine)

assert not [k for k in conftest.EXP_VARS if k in os.environ], "test switches set: this module runs the product library only"


@pytest.fixture(autouse=True)
def _product_only():
    assert not [k for k in conftest.EXP_VARS if k in os.environ]
    yield


# ------------------------------------------------------------------------------------------------------------------------ genomes

@pytest.fixture(scope="module")
def rep_genome(tmp_path_factory):
    """~100 kb in two sequences: random background, a 60-nt family planted 240 times (nine in ten copies with one substitution:
    many distinct strings per query, more than a 256-entry LDS list of k_search1s holds),
    a 24-nt family in 40 copies, a 300-nt poly-A stretch and a few N runs"""
    rng = random.Random(2024)
    unit = "".join(rng.choice("ACGT") for _ in range(60))
    unit2 = "".join(rng.choice("ACGT") for _ in range(24))
    seqs = []
    for c in range(2):
        s = bytearray(rng.choice(b"ACGT") for _ in range(50000))
        for k in range(120):
            u = list(unit)
            if rng.random() < 0.9:
                j = rng.randrange(60)
                u[j] = rng.choice([x for x in "ACGT" if x != u[j]])
            u = "".join(u)
            if k % 4 == 3:
                u = revcomp(u)
            p = 200 + k * 400 + rng.randrange(0, 300)
            s[p:p + 60] = u.encode()
        for k in range(20):
            p = 500 + k * 2400 + rng.randrange(0, 60)
            s[p:p + 24] = unit2.encode()
        s[30000 + c * 1000:30300 + c * 1000] = b"A" * 300
        for p in (12345, 40001):
            s[p:p + 5] = b"N" * 5
        seqs.append(s.decode())
    text = genome_text(seqs)
    path = str(tmp_path_factory.mktemp("hist") / "rep.fm9")
    O.build_fm9(text, path)
    # clean windows stay off the families and the poly-A: no 10-mer of them (a 20-mer across a copy with one substitution keeps one)
    avoid = {u[i:i + 10] for u in (unit, revcomp(unit), unit2, revcomp(unit2), "A" * 12, "T" * 12) for i in range(len(u) - 9)}
    return {"seqs": seqs, "text": text, "fm9": path, "seqlen": [len(s) + 1 for s in seqs], "names": ["r1", "r2"],
            "units": (unit, unit2), "avoid": avoid}


@pytest.fixture(scope="module")
def genomes(small_genome, rep_genome):
    return {"small": small_genome, "rep": rep_genome}


def open_product(g, monkeypatch, k=9, k2=None, **kw):
    """a fresh handle on the product library; the table orders through the deployment knobs DICEY_KMER_K / DICEY_KMER_K2"""
    monkeypatch.setenv("DICEY_KMER_K", str(k))
    if k2 is not None:
        monkeypatch.setenv("DICEY_KMER_K2", str(k2))
    try:
        ix = dicey_amd.FmIndex(g["fm9"], **kw)
    finally:
        monkeypatch.delenv("DICEY_KMER_K", raising=False)
        monkeypatch.delenv("DICEY_KMER_K2", raising=False)
    assert ix._L is _capi.load()
    return ix


# ------------------------------------------------------------------------------------------------------------------- batch kinds

def _window(g, rng, m, edits=0):
    while True:
        s = g["seqs"][rng.randrange(len(g["seqs"]))]
        p = rng.randrange(len(s) - m)
        q = s[p:p + m]
        if all(c in "ACGT" for c in q) and not any(q[i:i + 10] in g.get("avoid", ()) for i in range(m - 9)):
            break
    q = list(q)
    for _ in range(edits):
        k = rng.randrange(len(q))
        q[k] = rng.choice([x for x in "ACGT" if x != q[k]])
    q = "".join(q)
    return revcomp(q) if rng.random() < 0.3 else q


def _clean(g, rng, n, m=20):
    return [_window(g, rng, m, rng.choice([0, 0, 1])) if rng.random() < 0.8 else "".join(rng.choice("ACGT") for _ in range(m))
            for _ in range(n)]


def _with_n(q, rng):
    k = rng.choice([0, len(q) - 1, rng.randrange(1, len(q) - 1)])
    return q[:k] + "N" + q[k + 1:]


def _repeat_rich(g, rng, n):
    unit, unit2 = g["units"]
    out = []
    for i in range(n):
        src = unit if i % 4 else unit2
        p = rng.randrange(len(src) - 20 + 1)
        q = src[p:p + 20]
        if rng.random() < 0.3:
            k = rng.randrange(20)
            q = q[:k] + rng.choice([x for x in "ACGT" if x != q[k]]) + q[k + 1:]
        out.append(revcomp(q) if rng.random() < 0.3 else q)
    return out


def _make_kind(g, name):
    """(queries, hunt keyword arguments) of a named batch kind on genome g"""
    rng = random.Random(name)
    if name == "one":
        return _clean(g, rng, 1), dict(distance=1)
    if name == "clean20":
        return _clean(g, rng, 20), dict(distance=1)
    if name == "clean40":
        return _clean(g, rng, 40), dict(distance=1)
    if name == "clean300":
        return _clean(g, rng, 300), dict(distance=1)
    if name == "clean40_d3":
        return _clean(g, rng, 40), dict(distance=3)
    if name == "clean3000":
        return _clean(g, rng, 3000), dict(distance=1)
    if name == "n300":  # about 5 % with an N at either end or inside
        qs = _clean(g, rng, 300)
        for i in range(0, 300, 20):
            qs[i] = _with_n(qs[i], rng)
        return qs, dict(distance=1)
    if name == "mid33":  # 33-35 nt: the walker (above 31 nt) and the full-matrix verify (above 32 nt)
        return [_window(g, rng, rng.choice([33, 34, 35]), rng.choice([0, 1])) for _ in range(40)], dict(distance=1)
    if name == "mid33_2200":
        return [_window(g, rng, rng.choice([33, 34, 35]), rng.choice([0, 1])) for _ in range(2200)], dict(distance=1)
    if name == "long45":  # nothing packs: k_search1p
        qs = _clean(g, rng, 40)
        qs[17] = _window(g, rng, 45, 1)
        return qs, dict(distance=1)
    if name == "rep40":  # many hits, locate jobs, full LDS lists
        return _repeat_rich(g, rng, 40), dict(distance=1, max_locations=1000)
    if name == "rich40":  # every query from the 60-nt family: the most distinct occurring strings per workgroup
        unit = g["units"][0]
        qs = []
        for i in range(40):
            q = unit[i % 41:i % 41 + 20]
            qs.append(revcomp(q) if i % 3 == 2 else q)
        return qs, dict(distance=1, max_locations=1000)
    if name == "d2":
        return _clean(g, rng, 120), dict(distance=2)
    if name == "d2_short11":
        qs = _clean(g, rng, 40)
        for i in range(0, 40, 5):
            qs[i] = _window(g, rng, 11)
        return qs, dict(distance=2)
    if name == "d2_walker":  # N-bearing queries and a 42-nt one: walker groups, and nothing packs (k_search2p without select)
        qs = _clean(g, rng, 40)
        for i in range(0, 40, 6):
            qs[i] = _with_n(qs[i], rng)
        qs[13] = _window(g, rng, 42, 1)
        return qs, dict(distance=2, max_neighborhood=200000)
    if name == "d2_n":  # N-bearing 20-mers only: walker groups beside the fused kernel
        qs = _clean(g, rng, 40)
        for i in range(0, 40, 4):
            qs[i] = _with_n(qs[i], rng)
        return qs, dict(distance=2)
    if name == "d2_n_rich":  # N-bearing 20-mers and homopolymers (strings of more than 16 occurrences): walker and locate jobs
        qs = _clean(g, rng, 40)
        for i in range(0, 40, 4):
            qs[i] = _with_n(qs[i], rng)
        qs[5:9] = ["A" * 20, "C" * 20, "G" * 20, "T" * 20]
        return qs, dict(distance=2)
    if name == "ham1":
        return _clean(g, rng, 60), dict(distance=1, hamming=True)
    if name == "ham2":
        return _clean(g, rng, 60), dict(distance=2, hamming=True)
    if name == "fwd_m3":
        return _clean(g, rng, 40) + _repeat_rich(g, rng, 6), dict(distance=1, forward_only=True, max_locations=3)
    if name == "capped25":  # capped neighbourhoods: device enumeration, and an N-bearing one on the host
        qs = [_window(g, rng, 25, rng.choice([0, 1])) for _ in range(5)]
        qs.append(_with_n(_window(g, rng, 25), rng))
        return qs, dict(distance=2)
    raise KeyError(name)


_kinds, _answers, _orcs = {}, {}, {}


def kind(genomes, gname, name):
    key = (gname, name)
    if key not in _kinds:
        _kinds[key] = _make_kind(genomes[gname], name)
    return _kinds[key]


def answer(genomes, gname, name):
    """the checker's (json lines, hits per query) of a kind, worked out once per module"""
    key = (gname, name)
    if key not in _answers:
        g = genomes[gname]
        qs, kw = kind(genomes, gname, name)
        if gname not in _orcs:
            _orcs[gname] = O.Index(g["fm9"])
        O.fast_neighbors(True)
        try:
            _answers[key] = _orcs[gname].hunt_parallel(g["seqlen"], g["names"], qs, workers=min(CHECK_THREADS, len(qs)), **kw)
        finally:
            O.fast_neighbors(False)
    return _answers[key]


def check(genomes, gname, name, got, tag=""):
    qs, kw = kind(genomes, gname, name)
    lines, per = answer(genomes, gname, name)
    assert len(got.queries) == len(qs) == len(lines)
    ml, mn = kw.get("max_locations", 1000), kw.get("max_neighborhood", 10000)
    for qi, qr in enumerate(got.queries):
        a = [(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in qr.hits]
        assert a == per.get(qi, []), (tag, name, qi, qs[qi], len(a), len(per.get(qi, [])))
        assert qr.messages(ml, mn) == [e["title"] for e in json.loads(lines[qi])["errors"]], (tag, name, qi, qs[qi])
    return got


def run(ix, genomes, gname, name, tag="", **over):
    qs, kw = kind(genomes, gname, name)
    got = ix.hunt(qs, genomes[gname]["seqlen"], **dict(kw, **over))
    return check(genomes, gname, name, got, tag)


# ---------------------------------------------------------------------------------------------------------------- schedules

def test_generic_hint_rearms_and_decays(genomes, monkeypatch):
    """distance 1: a fresh handle's first clean batch runs the generic kernels (form 2), the next one not (3); an N-bearing batch
    after the hint decayed is repeated with them (2), the hint stays for STICKY clean batches, then form 3 again"""
    ix = open_product(genomes["small"], monkeypatch)
    forms = []
    for name in ["clean300", "clean300", "n300"] + ["clean300"] * (STICKY + 1):
        forms.append(run(ix, genomes, "small", name, tag=len(forms)).path["flat_kernel_form"])
    assert forms == [2, 3, 2] + [2] * STICKY + [3], forms
    ix.close()


def test_short_strings_leave_long2_for_sticky_batches(genomes, monkeypatch):
    """distance 2 with the long filter (order 10): 20-mers run the LONG2 body (7); a batch holding 11-mers is repeated with the r04
    body (5), which stays for STICKY batches; then LONG2 again.  Then the same while the walker and the locate jobs are on (sticky
    after N-bearing and repeat-rich batches): the short strings are the only reason left to repeat the batch"""
    ix = open_product(genomes["small"], monkeypatch, k=9, k2=10)
    forms = []
    for name in ["d2", "d2", "d2_short11"] + ["d2"] * (STICKY + 1):
        forms.append(run(ix, genomes, "small", name, tag=len(forms)).path["flat_kernel_form"])
    assert forms == [7, 7, 5] + [5] * STICKY + [7], forms
    forms = []
    for name in ["d2_n_rich", "d2_short11"] + ["d2_n_rich"] * STICKY + ["d2_short11", "d2"]:
        forms.append(run(ix, genomes, "small", name, tag=len(forms)).path["flat_kernel_form"])
    assert forms == [7, 5] + [5] * STICKY + [5, 5], forms
    ix.close()


def test_walker_rearms_after_clean_distance2_batches(genomes, monkeypatch):
    """distance 2: clean batches switch the walker off; a batch with N-bearing queries and a 42-nt query (nothing packs: no fused
    select, so only the walker branch can ask for the repeat) and one with N-bearing 20-mers beside the fused kernel must still
    find every hit"""
    ix = open_product(genomes["small"], monkeypatch)
    for _ in range(3):
        run(ix, genomes, "small", "d2")
    got = run(ix, genomes, "small", "d2_walker")
    assert got.path["flat_kernel_form"] in (4, 6), got.path
    assert got.path["cap_queries_device"] == got.path["cap_queries_host"] == got.path["cap_patterns"] == 0, got.path
    for _ in range(STICKY + 1):
        run(ix, genomes, "small", "d2")
    got = run(ix, genomes, "small", "d2_n")
    assert got.path["flat_kernel_form"] in (5, 7) and got.path["cap_patterns"] == 0, got.path
    for _ in range(3):
        run(ix, genomes, "small", "d2")
    ix.close()


def test_capacities_learnt_on_the_product_library(genomes, monkeypatch):
    """a fresh handle: a 20-query batch, then a repeat-rich batch with more hits than the fresh capacity 4 nq + 1024 (the hit
    retry; the counters show it), then 2 200 queries of 33-35 nt after a batch without walker groups: 4 400 strands for the walker
    against a list of 0 * 1.25 + 4 096 groups (hunt.hip walk_cap), so the list overflows and the batch is repeated.  That retry
    and the shard / flat slice retries have no observable in dg_hunt_result: only the answers are asserted for them."""
    ix = open_product(genomes["rep"], monkeypatch)
    run(ix, genomes, "rep", "clean20")
    got = run(ix, genomes, "rep", "rep40")
    assert got.counters["nhits"] > 4 * 40 + 1024, got.counters
    run(ix, genomes, "rep", "clean20")
    qs = kind(genomes, "rep", "mid33_2200")[0]
    assert 2 * sum(len(q) > 31 for q in qs) > 4096  # walker strands above the list a handle without walker history sizes
    run(ix, genomes, "rep", "mid33_2200")
    run(ix, genomes, "rep", "clean20")
    ix.close()


def test_verify_width_follows_history(genomes, monkeypatch):
    """the same clean batch before and after a hit-heavy one: k_verify_memo goes from 1 hit per lane to 4 or 8, same answers"""
    ix = open_product(genomes["rep"], monkeypatch)
    a = run(ix, genomes, "rep", "clean300")
    run(ix, genomes, "rep", "rep40")
    b = run(ix, genomes, "rep", "clean300")
    assert a.path["verify_kernel_form"] & 0xff == 1, a.path
    assert b.path["verify_kernel_form"] & 0xff in (4, 8), b.path
    assert a.path["verify_kernel_form"] >> 8 == b.path["verify_kernel_form"] >> 8 == 7
    assert [q.hits for q in a.queries] == [q.hits for q in b.queries]
    ix.close()


def test_lds_list_hand_over(genomes, monkeypatch):
    """k_search1s' LDS list follows history: 256 entries after clean batches, 512 after a batch that averaged more than 48 occurring
    strings per workgroup.  After clean batches the family's 20-mers overflow the 256-entry list: their groups are handed to the
    generic kernels and the batch is repeated (form 2; no N, no query above 31 nt, so nothing else asks for the generic kernels).
    Repeated on the 512-entry list the same batch fits: once the generic hint has decayed it runs on form 3 again."""
    ix = open_product(genomes["rep"], monkeypatch)
    names = ["clean40", "clean40", "rich40"] + ["rich40"] * STICKY + ["rich40", "clean40", "rep40", "clean40"]
    forms = [run(ix, genomes, "rep", n, tag=k).path["flat_kernel_form"] for k, n in enumerate(names)]
    assert forms[:3] == [2, 3, 2], forms  # 256-entry list overflows: hand-over and repeat
    assert forms[3 + STICKY] == 3, forms  # 512-entry list holds the same batch
    ix.close()


def test_locate_job_hint_decays_then_rearms(genomes, monkeypatch):
    """nine batches without strings of more than 16 occurrences, then a repeat-rich one (queued jobs, repeated with the job kernels)"""
    ix = open_product(genomes["rep"], monkeypatch)
    for _ in range(STICKY + 1):
        run(ix, genomes, "rep", "clean40")
    run(ix, genomes, "rep", "rep40")
    run(ix, genomes, "rep", "clean40")
    ix.close()


def test_classic_fetch_follows_history(genomes, monkeypatch):
    """compact=False: few hits, many (the speculative copy is too short: copied again), few again, interleaved with compact batches"""
    ix = open_product(genomes["rep"], monkeypatch)
    for name, compact in [("clean40", False), ("rep40", False), ("clean40", False), ("rep40", True), ("clean40", False),
                          ("rep40", False), ("rep40", False), ("clean300", True), ("clean40", False)]:
        run(ix, genomes, "rep", name, tag=(name, compact), compact=compact)
    ix.close()


def test_refusals_mid_stream(genomes, monkeypatch):
    """every refused call is followed by a batch that must still match"""
    import ctypes as C
    import torch
    g = genomes["small"]
    ix = open_product(g, monkeypatch)
    run(ix, genomes, "small", "clean300")
    qs = kind(genomes, "small", "clean20")[0]
    with pytest.raises(dicey_amd.DgError):
        ix.hunt(qs, g["seqlen"], distance=30)
    run(ix, genomes, "small", "n300")
    with pytest.raises(dicey_amd.DgError):
        ix.hunt(qs[:3] + ["ACGT" * 8000], g["seqlen"], distance=1)
    run(ix, genomes, "small", "clean300")
    capped = kind(genomes, "small", "capped25")[0][:5]
    monkeypatch.setenv("DICEY_CAP_BUDGET_MB", "1")
    try:
        with pytest.raises(dicey_amd.DgError):
            ix.hunt(capped, g["seqlen"], distance=2)
    finally:
        monkeypatch.delenv("DICEY_CAP_BUDGET_MB")
    run(ix, genomes, "small", "capped25")
    with pytest.raises(dicey_amd.DgError) as e:
        ix.hunt([], g["seqlen"], distance=1)
    assert e.value.code == -1  # DG_EINVAL
    run(ix, genomes, "small", "d2")
    # dg_hunt_device with offsets that decrease: refused on the host before any kernel
    qb = "".join(qs[:3]).encode()
    d_q = torch.frombuffer(bytearray(qb), dtype=torch.uint8).cuda()
    d_off = torch.tensor([0, 40, 20, 60], dtype=torch.int64).cuda()
    sl = (C.c_uint32 * len(g["seqlen"]))(*g["seqlen"])
    p = _capi.HuntParams(1, 0, 0, 1000, 10000, 0, _capi.DG_HUNT_COMPACT)
    rp = C.POINTER(_capi.HuntResult)()
    rc = ix._L.dg_hunt_device(ix.handle, C.byref(p), sl, len(g["seqlen"]), C.c_void_p(d_q.data_ptr()), C.c_void_p(d_off.data_ptr()),
                              3, len(qb), 1, C.byref(rp))
    assert rc != 0
    run(ix, genomes, "small", "clean300")
    run(ix, genomes, "small", "clean300")
    ix.close()


def test_other_entry_points_between_hunts(genomes, monkeypatch):
    """count / locate / extract, neighborhood_count (run_batch in count mode) and mappability between hunt batches of one handle"""
    import numpy as np
    import mappability_ref as MR
    g = genomes["small"]
    ix = open_product(g, monkeypatch)
    orc = O.Index(g["fm9"])
    pats = [q.encode() for q in kind(genomes, "small", "clean20")[0][:10]]
    run(ix, genomes, "small", "clean300")
    assert ix.count(pats) == [orc.count(p) for p in pats]
    run(ix, genomes, "small", "n300")
    assert [sorted(x) for x in ix.locate(pats)] == [sorted(orc.locate(p)) for p in pats]
    run(ix, genomes, "small", "clean300")
    assert ix.extract([(5, 40), (30100, 30150)]) == [orc.extract(5, 40), orc.extract(30100, 30150)]
    run(ix, genomes, "small", "d2")
    arms = [_window(g, random.Random(3), 20) for _ in range(6)]
    nc = ix.neighborhood_count([a.encode() for a in arms], distance=1)
    for a, (fw, rv) in zip(arms, nc):
        assert fw == sum(orc.count(s.encode()) for s in O.neighbors(a, 1, True, 10000)), a
        assert rv == sum(orc.count(s.encode()) for s in O.neighbors(revcomp(a), 1, True, 10000)), a
    run(ix, genomes, "small", "clean300")
    m = ix.mappability(k=20)
    assert np.array_equal(m, MR.values(g["text"], 20, forward_only=False))
    run(ix, genomes, "small", "n300")
    run(ix, genomes, "small", "d2")
    ix.close()


@pytest.mark.skipif(O.ref_libs() is None, reason="oracle/_ref (the reference's thal() build) not present")
def test_search_sites_between_hunts(genomes, monkeypatch):
    """search_sites (run_batch with its site stage) between hunt batches of one handle: the same sites as on a fresh handle, and
    every primer's Tm against its perfect complement equal to the reference thal()"""
    import ctypes as C
    g = genomes["small"]
    rng = random.Random(31)
    primers = [_window(g, rng, rng.choice([18, 20, 22]), rng.choice([0, 0, 1])) for _ in range(24)]
    th = dicey_amd.Thal(O.PRIMER3_CONFIG)
    fresh = open_product(g, monkeypatch)
    want = dicey_amd.search_sites(fresh, th, primers, g["seqlen"])
    fresh.close()
    assert want[0]
    T, _ = O.ref_libs()
    T.ref_thal.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    t, a, b = C.c_double(), C.c_int(), C.c_int()
    for p, m in zip(primers, want[1]):
        T.ref_thal(p.encode(), revcomp(p).encode(), C.byref(t), C.byref(a), C.byref(b))
        assert t.value == m, p
    ix = open_product(g, monkeypatch)
    for name in ("clean300", "n300", "d2_walker"):
        run(ix, genomes, "small", name)
        assert dicey_amd.search_sites(ix, th, primers, g["seqlen"]) == want, name
    run(ix, genomes, "small", "clean300")
    run(ix, genomes, "small", "d2")
    ix.close()
    th.close()


def _submit_schedule(ix, genomes, gname, names, inflight=3):
    """the batches of a schedule through hunt_submit / hunt_wait, `inflight` at a time on one handle: answers only"""
    open_ = []
    for name in names:
        if len(open_) == inflight:
            n0, t0 = open_.pop(0)
            check(genomes, gname, n0, ix.hunt_wait(t0), tag="lanes")
        qs, kw = kind(genomes, gname, name)
        open_.append((name, ix.hunt_submit(qs, genomes[gname]["seqlen"], **kw)))
    for n0, t0 in open_:
        check(genomes, gname, n0, ix.hunt_wait(t0), tag="lanes")


def test_schedules_on_lanes(genomes, monkeypatch):
    """the schedules above with three batches in flight on one handle (the lanes merge their hints; the forms depend on timing)"""
    ix = open_product(genomes["small"], monkeypatch, k=9, k2=10)
    _submit_schedule(ix, genomes, "small", ["clean300", "clean300", "n300"] + ["clean300"] * (STICKY + 1))
    _submit_schedule(ix, genomes, "small", ["d2", "d2", "d2_short11"] + ["d2"] * (STICKY + 1) + ["d2_walker", "d2_n", "d2"])
    ix.close()
    ix = open_product(genomes["rep"], monkeypatch)
    _submit_schedule(ix, genomes, "rep", ["clean20", "rep40", "clean300", "mid33_2200", "clean300", "rep40", "clean40"] +
                     ["clean40"] * (STICKY + 1) + ["rep40", "clean300"])
    ix.close()


RANDOM_POOL = ["one", "clean40", "clean300", "clean3000", "n300", "mid33", "long45", "rep40", "d2", "d2_short11", "d2_walker", "d2_n",
               "d2_n_rich", "ham1", "ham2", "fwd_m3", "capped25"]


def test_seeded_random_history(genomes, monkeypatch):
    """60 batches drawn from the pool in a fixed order on one handle, blocking calls mixed with up to three submissions in flight;
    the pool holds batches of 1, ~40, a few hundred and 3 000 queries, so the handle keeps meeting batches larger than it learnt from"""
    rng = random.Random(606)
    ix = open_product(genomes["rep"], monkeypatch)
    g = genomes["rep"]
    open_ = []
    for step in range(60):
        name = rng.choice(RANDOM_POOL)
        qs, kw = kind(genomes, "rep", name)
        if rng.random() < 0.5:
            if len(open_) == 3:
                n0, t0 = open_.pop(0)
                check(genomes, "rep", n0, ix.hunt_wait(t0), tag=("random", step))
            open_.append((name, ix.hunt_submit(qs, g["seqlen"], **kw)))
        else:
            for n0, t0 in open_:  # a blocking call waits for the batches in flight
                check(genomes, "rep", n0, ix.hunt_wait(t0), tag=("random", step))
            open_ = []
            check(genomes, "rep", name, ix.hunt(qs, g["seqlen"], **kw), tag=("random", step))
    for n0, t0 in open_:
        check(genomes, "rep", n0, ix.hunt_wait(t0), tag="random-end")
    ix.close()


# ------------------------------------------------------------------------------------------- product paths of the forced switches

def test_product_path_unpacked_distance1(genomes, monkeypatch):
    """nofuse: a 45-nt query in a distance-1 batch: nothing packs, k_search1p (form 1); the 33-35-nt batch takes the full-matrix
    verify (noband: verify_kernel_form 0), and so does distance 3"""
    ix = open_product(genomes["small"], monkeypatch)
    assert run(ix, genomes, "small", "long45").path["flat_kernel_form"] == 1
    got = run(ix, genomes, "small", "mid33")
    assert got.path["verify_kernel_form"] == 0 and got.path["flat_kernel_form"] in (2, 3), got.path
    got = run(ix, genomes, "small", "clean40_d3")
    assert got.path["verify_kernel_form"] == 0 and got.path["flat_kernel_form"] == 0, got.path
    assert run(ix, genomes, "small", "clean40").path["verify_kernel_form"] >> 8 == 7
    ix.close()


def test_product_path_distance2_without_fused_select(genomes, monkeypatch):
    """nofuse2 / nopre5d2: a distance-2 batch with a 42-nt query runs k_search2p without the select stage (form 4 or 6)"""
    ix = open_product(genomes["small"], monkeypatch)
    assert run(ix, genomes, "small", "d2_walker").path["flat_kernel_form"] in (4, 6)
    assert run(ix, genomes, "small", "d2").path["flat_kernel_form"] in (5, 7)
    ix.close()


def test_product_path_without_long_filter(genomes, monkeypatch):
    """nolong2: DICEY_KMER_K2=0 opens without the long filter; every distance-2 batch then runs the r04 body (form 5)"""
    ix = open_product(genomes["small"], monkeypatch, k=9, k2=0)
    for name in ("d2", "d2_short11", "d2_n", "d2"):
        assert run(ix, genomes, "small", name).path["flat_kernel_form"] == 5
    ix.close()


def test_product_path_compact_open_hamming(genomes, monkeypatch):
    """nodirectctx: the compact open (no pre5 / context records) with Hamming mode and distance 2 on the repeat-rich genome"""
    ix = open_product(genomes["rep"], monkeypatch, compact=True, pre5=False)
    for name in ("ham1", "ham2", "d2", "rep40", "clean300", "ham1"):
        run(ix, genomes, "rep", name)
    ix.close()


def test_product_path_cap_device_and_host(genomes, monkeypatch):
    """caphost: capped 25-mers are enumerated on the device, the N-bearing one on the host, in one batch"""
    ix = open_product(genomes["small"], monkeypatch)
    got = run(ix, genomes, "small", "capped25")
    assert got.path["cap_queries_device"] > 0 and got.path["cap_queries_host"] > 0, got.path
    run(ix, genomes, "small", "clean300")
    ix.close()
