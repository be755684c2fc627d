"""The search and select stages of `dicey hunt` (hunt_search.hpp: k_search1s, k_search2p<true, .>; hunt_select.hpp: k_group_pack,
k_group_select, k_leaf_alive, k_leaf_rank, k_group, k_select, k_take) on the saturated texts of tests/select_shapes.py: an LDS list of
one workgroup with 0, 1, 64, 65, 256, 257, 512 and 513 occurring strings, a Sel slice with 64 and 65 kept strings, saturated groups in
the first and the last slot of a workgroup and split across two, low-complexity queries with every candidate planted, queries of 41
and 42 nt, and at distance 2 a group of 512 / 513 and of 1 024 / 1 025 occurring strings.

Every case is seen through two observables: count mode (FmIndex.neighborhood_count: search and select with nothing behind them) per
query and strand against the sum of the oracle's counts over the reference's neighbourhood, and hunt hit by hit in the reference's
push order (_compare), with max_locations above the total and ending inside the forward and inside the reverse strand's strings.
Every hunt also states which flat kernel ran (flat_kernel_form) and, where the case has an exact census, how many occurring strings
the search stage emitted (the `leaves` counter): tests/test_select_shapes_host.py derived both numbers' expectations from the
reference side; the library's word only confirms that the run reached the occupancy it was built for."""
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import dicey_amd
import select_shapes as S
from test_gpu_locate_topk import _compare

pytestmark = pytest.mark.gpu
MODES = [pytest.param(False, id="edit"), pytest.param(True, id="hamming")]


@pytest.fixture(scope="module", autouse=True)
def table_orders():
    """every handle of this module opens with the same table and filter orders, whatever the text's size"""
    mp = pytest.MonkeyPatch()
    mp.setenv("DICEY_KMER_K", str(S.K))
    mp.setenv("DICEY_KMER_K2", str(S.K2))
    yield
    mp.undo()


@pytest.fixture(scope="module")
def fm9(tmp_path_factory):
    d = tmp_path_factory.mktemp("select_shapes")
    built = {}

    def path(name):
        if name not in built:
            built[name] = str(d / (name + ".fm9"))
            dicey_amd.build_index(S.genome(name)["text"], built[name])   # the GPU builder (byte-identical to the oracle's, tests/test_gpu_parity.py)
        return built[name]
    return path


def count_mode(h, name, batch, ham):
    """FmIndex.neighborhood_count per query and strand against the oracle's counts summed over the reference's neighbourhood"""
    g, ref = S.genome(name), S.reference(name)
    got = h.neighborhood_count([q.encode() for q in batch["qs"]], distance=g["d"], hamming=ham)
    want = ref.sums(batch["qs"], g["d"], ham)
    bad = [(i, batch["qs"][i], a, b) for i, (a, b) in enumerate(zip(got, want)) if tuple(a) != tuple(b)]
    assert not bad, bad[:4]
    return want


def hunt(h, name, batch, ham, form, leaves=None, limits=None):
    """hit by hit at every limit; the flat kernel's form and the search stage's census at each"""
    g, ref = S.genome(name), S.reference(name)
    out = []
    total = [a + b for a, b in ref.sums(batch["qs"], g["d"], ham)]
    for m in limits or S.limits(ref, batch, g["d"], ham):
        got = _compare(h, ref, g, batch["qs"], distance=g["d"], hamming=ham, max_locations=m)
        assert got.path["flat_kernel_form"] == form, (m, got.path)
        if leaves is not None:
            assert got.counters["leaves"] == leaves, (m, got.counters)
        assert [len(q.hits) for q in got.queries] == [min(t, m) for t in total], m    # every occurrence of a kept string is a hit, up to the limit
        out.append(got)
    return out


def pads_of(batch):
    """the batch's padding alone: nothing of it occurs"""
    return dict(batch, qs=[q for i, q in enumerate(batch["qs"]) if i not in batch["sat"]], sat=[], L={}, leaves=0)


def settle(h, name, batch, ham):
    """A handle's first batch runs with the generic kernels (Hints::generic starts at 1: hunt_hints.hpp); a batch that has no work for
    them turns them off for the next one.  The batch's own padding is that batch: form 2 at distance 1 (k_take a launch of its own),
    the LONG2 body at distance 2."""
    hunt(h, name, pads_of(batch), ham, 2 if S.genome(name)["d"] == 1 else 7, 0, limits=[1000])


def fresh(fm9, name, batch, ham, form, leaves=None):
    """count mode on a fresh handle (generic kernels on); the hunts on a fresh handle whose generic kernels one batch of padding has
    turned off, so that a workgroup or group that needs them repeats the batch"""
    with dicey_amd.FmIndex(fm9(name)) as h:
        sums = count_mode(h, name, batch, ham)
    with dicey_amd.FmIndex(fm9(name)) as h:
        settle(h, name, batch, ham)
        hunt(h, name, batch, ham, form, leaves)
    return sums


def occ(ham):
    return "occ_ham" if ham else "occ_edit"


# ---- distance 1: k_search1s ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ham", MODES)
def test_a_empty_and_single_string_workgroups(fm9, ham):
    """L = 0 (every group empty: nsel 0, selbase still set; with the generic kernels and, the second time, in the TAKE form) and L = 1"""
    b = S.genome(occ(ham))["batches"]
    assert fresh(fm9, occ(ham), b["a0"], ham, 3, 0) == [(0, 0)] * 24
    sums = fresh(fm9, occ(ham), b["a1"], ham, 3, 1)
    assert sum(a + c for a, c in sums) >= 1


@pytest.mark.parametrize("label,n", [("b64", 64), ("b65", 65)])
@pytest.mark.parametrize("ham", MODES)
def test_b_select_by_one_wavefront_or_by_four(fm9, ham, label, n):
    """64 occurring strings of a workgroup are selected by its first wavefront, 65 by all four (sstep)"""
    fresh(fm9, occ(ham), S.genome(occ(ham))["batches"][label], ham, 3, n)


@pytest.mark.parametrize("ham", MODES)
def test_c_the_list_of_256_holds_256_and_hands_257_over(fm9, ham):
    """256 fit a fresh handle's list (TAKE form); with 257 the workgroup's groups go to the generic kernels, which the fresh handle had
    left out: the batch runs again with them (form 2) — the same hits and sums either way"""
    b = S.genome(occ(ham))["batches"]
    s256 = fresh(fm9, occ(ham), b["c256"], ham, 3, 256)
    s257 = fresh(fm9, occ(ham), b["c257"], ham, 2, 257)
    x = b["c257"]["sat"][-1]
    assert s257[:x] == s256[:x] and sum(s257[x]) >= 1


@pytest.mark.parametrize("ham", MODES)
def test_d_the_list_of_512_holds_512_and_hands_513_over_in_rounds(fm9, ham):
    """right behind a batch whose census was 513 the list has 512 entries (Hints::fused_leaves): 512 fit; 513 overflow, and with more than
    512 survivors the workgroup sends its leaves out through the multi-round queue"""
    name = occ(ham)
    b = S.genome(name)["batches"]
    top = S.limits(S.reference(name), b["d513"], 1, ham)
    with dicey_amd.FmIndex(fm9(name)) as h:
        hunt(h, name, b["d513"], ham, 2, 513, top[:1])        # the fresh handle's list of 256 overflows: generic kernels from here on
        hunt(h, name, b["d512"], ham, 2, 512, top[:1])
        hunt(h, name, b["d513"], ham, 2, 513, top[:1])
        s512 = count_mode(h, name, b["d512"], ham)
        s513 = count_mode(h, name, b["d513"], ham)
        hunt(h, name, b["d512"], ham, 2, 512, top[1:])
        hunt(h, name, b["d513"], ham, 2, 513, top[1:])
    x = b["d513"]["sat"][-1]
    assert s513[:x] == s512[:x] and sum(s513[x]) >= 1


@pytest.mark.parametrize("label,n", [("e64", 64), ("e65", 65)])
@pytest.mark.parametrize("ham", MODES)
def test_e_a_sel_slice_of_64_holds_64_kept_strings_and_grows_for_65(fm9, ham, label, n):
    """a fresh handle's slices hold 64 kept strings; 65 of one workgroup overflow its slice (room) and the batch repeats with more"""
    b = S.genome(occ(ham))["batches"][label]
    assert sum(b["kept"].values()) == n and S.flat_cap(len(b["qs"])) == 64
    fresh(fm9, occ(ham), b, ham, 3, n)


@pytest.mark.parametrize("m", S.LAY_LENGTHS)
@pytest.mark.parametrize("ham", MODES)
def test_f_saturated_groups_in_the_first_and_last_slot_and_across_workgroups(fm9, ham, m, monkeypatch):
    """16 nt (gpw 16), 17 (gpw 14 in the TAKE form, 15 without: a query split across two workgroups), 31 (gpw 8), K + 1 (the shortest
    the flat kernel takes): the TAKE form, count mode, and the form with k_take a launch of its own (development build)"""
    from conftest import exp_lib
    name = "lay_ham" if ham else "lay_edit"
    b = S.genome(name)["batches"]["f%d" % m]
    fresh(fm9, name, b, ham, 3, 46)
    monkeypatch.setenv("DICEY_NO_PREP_FUSION", "1")
    with dicey_amd.FmIndex(fm9(name), _lib=exp_lib()) as h:
        settle(h, name, b, ham)
        hunt(h, name, b, ham, 2, 46)


@pytest.mark.parametrize("ham", MODES)
def test_g_low_complexity_queries_with_every_candidate_planted(fm9, ham):
    """a homopolymer run, a dinucleotide repeat, equal first and last characters; all candidates and the queries themselves occur"""
    fresh(fm9, "low", S.genome("low")["batches"][ham], ham, 3)


@pytest.mark.parametrize("m,form", [(41, 2), (42, 1)])
@pytest.mark.parametrize("ham", MODES)
def test_h_queries_of_41_and_42_nt(fm9, ham, m, form):
    """the walker's leaves through k_group_pack / k_leaf_alive / k_leaf_rank (41 nt: packed, beside k_search1s after one repeat) and
    through k_group / k_select (42 nt: beside k_search1p)"""
    fresh(fm9, "long", S.genome("long")["batches"][m, ham], ham, form)


# ---- distance 2: k_search2p<true, .> and the generic select behind it -------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("ham2_i", 512), ("ham2_i", 513), ("ham2_j1024", 1024), ("ham2_j1025", 1025)])
def test_i_j_hamming_groups_at_the_list_and_at_the_group_select_capacity(fm9, name, n):
    """512 fit k_search2p's list, 513 are searched again with their leaves written out; k_group_select takes a group of 1 024 leaves,
    k_leaf_alive / k_leaf_rank one of 1 025"""
    b = S.genome(name)["batches"][n]
    assert b["L"] == {6: n, 7: S.REV2}
    fresh(fm9, name, b, True, 7, n + S.REV2)


@pytest.mark.parametrize("body,form", [("long2", 7), ("r04", 5)])
@pytest.mark.parametrize("n", [513, 400])
def test_k_edit_distance_two_either_side_of_the_list(fm9, n, body, form):
    """at least 513 occurring candidates (the group goes to the generic select), and 400 that stay in the list — the leaf counter
    must say so; both bodies of k_search2p (a 15-mer in the batch keeps the LONG2 body away)"""
    g = S.genome("edit2")
    b = g["batches"][n, body]
    lo, hi = S.bracket(g, b)
    with dicey_amd.FmIndex(fm9("edit2")) as h:
        count_mode(h, "edit2", b, False)
    with dicey_amd.FmIndex(fm9("edit2")) as h:
        settle(h, "edit2", dict(b, qs=[q for q in b["qs"] if q != g["short"]], sat=[3]), False)
        for got in hunt(h, "edit2", b, False, form):
            leaves = got.counters["leaves"]
            print("edit2 %d %s: %d leaves (%d distinct occurring candidates, %d with the walk's duplicates)" % (n, body, leaves, lo, hi))
            assert lo <= leaves
            assert (leaves <= S.FUSED2_LCAP) == (n == 400)
