"""The cap stage of `dicey hunt` (hunt_cap.hpp: k_cap_enum; hunt.hip: cap_scan; hunt_search.hpp: k_explicit; the explicit-leaf paths of
hunt_select.hpp) on the saturated texts of tests/cap_shapes.py: every string of the reference's capped set occurs there, and so do
strings of the uncapped language outside it, so a set with one string missing, one too many, taken at the wrong rank or for the wrong
strand answers other hits.

Every run of a case is seen through: hunt hit by hit in the reference's push order (_compare) at each max_locations of the case, the
per-query messages and the DG_Q_NBHD_EXCEEDED flag against the oracle, the stage's own account (cap_queries_device, cap_queries_host,
cap_patterns) against the model of tests/cap_shapes.py, and count mode (FmIndex.neighborhood_count) per query and strand against the
oracle's counts summed over the capped set.  Cases 1 to 5 and 7 run on the product library (k_cap_enum) and on the development library
with DICEY_CAP_HOST (the host enumerator on the same texts); case 6 never qualifies for the device and runs on the product library."""
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import cap_shapes as C
import dicey_amd
from dicey_amd import DG_Q_NBHD_EXCEEDED
from test_gpu_locate_topk import _compare

pytestmark = pytest.mark.gpu
PATHS = ["device", "host"]


@pytest.fixture(scope="module", autouse=True)
def table_orders():
    """every handle of this module opens with the same table and filter orders, whatever the text's size"""
    mp = pytest.MonkeyPatch()
    mp.setenv("DICEY_KMER_K", str(C.K))
    mp.setenv("DICEY_KMER_K2", str(C.K2))
    yield
    mp.undo()


@pytest.fixture(scope="module")
def fm9(tmp_path_factory):
    d = tmp_path_factory.mktemp("cap_shapes")
    built = {}

    def path(name):
        if name not in built:
            built[name] = str(d / (name + ".fm9"))
            dicey_amd.build_index(C.case(name)["text"], built[name])   # the GPU builder (byte-identical to the oracle's, tests/test_gpu_parity.py)
        return built[name]
    return path


@pytest.fixture
def opened(fm9, monkeypatch):
    """open(case, path): a fresh handle on the product library, or on the development library with DICEY_CAP_HOST set"""
    hs = []

    def get(name, path="device"):
        lib = None
        if path == "host":
            from conftest import exp_lib
            monkeypatch.setenv("DICEY_CAP_HOST", "1")
            lib = exp_lib()
        hs.append(dicey_amd.FmIndex(fm9(name), _lib=lib))
        return hs[-1]
    yield get
    for h in hs:
        h.close()


def check(h, name, run, path="device"):
    c, ref, kw = C.case(name), C.reference(name), run["kw"]
    want = C.expect(run, host_only=path == "host")
    cap = kw["max_neighborhood"]
    for ml in C.limits(ref, run):
        got = _compare(h, ref, c, run["qs"], max_locations=ml, **kw)
        titles = ref.titles(run["qs"], max_locations=ml, **kw)
        for qi, qr in enumerate(got.queries):
            assert qr.messages(ml, cap) == titles[qi], (name, run["label"], ml, qi, run["qs"][qi])
            assert bool(qr.flags & DG_Q_NBHD_EXCEEDED) == want["fired"][qi], (name, run["label"], ml, qi, run["qs"][qi])
        account = (got.path["cap_queries_device"], got.path["cap_queries_host"], got.path["cap_patterns"])
        assert account == (want["device"], want["host"], want["patterns"]), (name, run["label"], ml, got.path)
    if run["count"]:
        d, ham = kw["distance"], kw.get("hamming", False)
        qs = [q for q in run["qs"] if len(q) >= 10]       # (dg_neighborhood_count takes sequences of 10 nt and more)
        counts = h.neighborhood_count([q.encode() for q in qs], distance=d, hamming=ham, max_neighborhood=cap)
        sums = ref.sums(qs, d, ham, cap)
        bad = [(i, qs[i], a, b) for i, (a, b) in enumerate(zip(counts, sums)) if tuple(a) != tuple(b)]
        assert not bad, (name, run["label"], bad[:4])
        for i in run["sat"]:      # on these texts every term is non-zero: the sum holds every string of the set at least once
            q = run["qs"][i]
            for s, total in zip(C.strands(q), sums[qs.index(q)]):
                assert total >= len(C.capped(s, d, ham, cap))
    return want


def labels(name):
    return [r["label"] for r in C.case(name)["runs"]]


def queries_of(name):
    return list(dict.fromkeys(r["qs"][0] for r in C.case(name)["runs"]))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("qi", range(6))
def test_1_distance_one_at_every_cap_edge(opened, path, qi):
    """10, 20 and 30 nt, random and low-complexity: max_neighborhood 1, 2, 17, F - 1, F, F + 1 on one handle"""
    q = queries_of("c1")[qi]
    h = opened("c1", path)
    fired = [check(h, "c1", r, path)["fired"][0] for r in C.case("c1")["runs"] if r["qs"][0] == q]
    assert len(fired) == 6 and all(fired[:5])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("qi", range(4))
def test_2_distance_two_at_every_cap_edge(opened, path, qi):
    """10 and 12 nt: max_neighborhood 2, 50, F // 2, F - 1, F, F + 1; and a cap that fires on the forward / on the reverse strand alone
    (the silent strand's whole set travels beside the capped one)"""
    q = queries_of("c2_small")[qi]
    h = opened("c2_small", path)
    runs = [r for r in C.case("c2_small")["runs"] if r["qs"][0] == q]
    assert len(runs) == (6 if qi < 2 else 1)
    for r in runs:
        check(h, "c2_small", r, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("label", ["m29/x64", "m29/x10000"])
def test_2_the_longest_key_at_64_and_at_the_default_cap(opened, path, label):
    assert check(opened("c2_m29", path), "c2_m29", C.run_of("c2_m29", label), path)["fired"] == [True]


@pytest.mark.parametrize("path", PATHS)
def test_2_the_shortest_length_the_default_cap_looks_at(opened, path):
    """21 nt: enumerated, silent, left to the search kernels with its whole set occurring"""
    want = check(opened("c2_m21", path), "c2_m21", C.run_of("c2_m21", "m21/x10000"), path)
    assert want["fired"] == [False] and want["patterns"] == 0


@pytest.mark.parametrize("path", PATHS)
def test_3_the_qualification_edge_lower_case_and_forward_only(opened, path):
    h = opened("c3", path)
    for label in labels("c3"):
        check(h, "c3", C.run_of("c3", label), path)
    r = C.run_of("c3", "case/20")
    got = h.hunt(r["qs"], C.case("c3")["seqlen"], max_locations=100000, **r["kw"])
    upper, lower = ([(x.score, x.chr, x.start, x.strand, x.refalign, x.queryalign) for x in q.hits] for q in got.queries)
    assert upper == lower and len(upper) >= 2 * 17


@pytest.mark.parametrize("path", PATHS)
def test_4_more_jobs_than_persistent_workgroups_then_a_smaller_batch(opened, path):
    """1 100 jobs on 1 024 workgroups: 76 of them clear their tables, events and filter for a 10-mer behind a 30-mer; then twelve
    12-mers at distance 2 on the same handle"""
    h = opened("c4", path)
    want = check(h, "c4", C.run_of("c4", "d1/1100"), path)
    assert all(want["fired"])
    check(h, "c4", C.run_of("c4", "d2/12"), path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("where", ["alone", "at40"])
@pytest.mark.parametrize("which", range(3))
def test_5_a_group_of_a_thousand_occurring_explicit_strings(opened, path, where, which):
    """SELCAP and SELCAP + 1 occurring explicit strings in one group, alone and as query 40 of 65, max_locations above the total and
    inside either strand's strings.  (The result does not say how many attempts the batch took: the answer is the oracle's.)"""
    runs = [r for r in C.case("c5")["runs"] if r["label"].startswith(where)]
    assert [r["kw"]["max_neighborhood"] for r in runs][:2] == [C.S.SELCAP, C.S.SELCAP + 1] and len(runs) == 3    # (F = 1 278 for this query)
    check(opened("c5", path), "c5", runs[which], path)


@pytest.mark.parametrize("label", ["two_n", "hamming2", "m41", "m42", "m43", "m41-43"])
def test_6_host_path_explicit_strings(opened, label):
    """strings with N, Hamming distance 2, strings of 40 to 44 characters: on the product library"""
    want = check(opened("c6"), "c6", C.run_of("c6", label))
    assert want["device"] == 0 and all(want["fired"])


@pytest.mark.parametrize("path", PATHS)
def test_7_a_mixed_batch(opened, path):
    check(opened("c7", path), "c7", C.run_of("c7", "mixed"), path)
