"""tests/search_queue_shapes.py from the reference side, without a GPU: every case's text is recounted from scratch — candidates whose
last window occurs, whose first window occurs as well, whose whole string occurs — over every query of its batch, and held against the
census the case was built for and against the two counters the search stage reports (ctr_filter_probes, ctr_leaves) as recorded from
the parent of the commit that moved the head probe in front of k_search1s's queue.  A case that cannot be built fails here."""
import pytest

import search_queue_shapes as Q
import select_shapes as S


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_every_case_builds_and_its_census_holds_on_the_finished_text(name):
    g = Q.case(name)
    c = Q.census(g)
    want = g["want"]
    assert c["per_wg"][1] == (want["tail_only"], want["both"], want["occurring"]), c["per_wg"]
    # the padding's workgroups: nothing occurs (a window of a padding candidate may: the texts have up to 35 000 of them, and the
    # counters' expectations come from the census of the whole batch)
    assert set(c["per_wg"]) == {0, 1, 2} and c["per_wg"][0][2] == 0 and c["per_wg"][2][2] == 0, c["per_wg"]
    assert c["occurring"] == want["occurring"]
    assert "N" not in "".join(g["qs"]) and {len(q) for q in g["qs"]} == {g["m"]}
    assert S.gpw_of(g["m"], True) == S.gpw_of(g["m"], False)                           # one layout for both kernel forms


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_probe_formula_against_the_parents_counters(name):
    """ctr_filter_probes = (valid candidates, each asks a filter) + (tail-window survivors longer than K2); ctr_leaves = the census of
    occurring candidates"""
    assert name in Q.PARENT_COUNTERS, "no counters recorded for this case"
    c = Q.census(Q.case(name))
    assert (Q.probes(c), c["occurring"]) == tuple(Q.PARENT_COUNTERS[name][:2])


def test_the_double_survivor_series_sits_on_the_kernels_boundaries():
    assert Q.T_LEAVE == 64 and Q.T_OTHER == 256 and Q.FUSED_QCAP == S.FUSED_QCAP
    for n in (0, 1, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513):
        g = Q.case("double%d" % n)
        assert g["want"]["both"] == n
        # three tail-only survivors per double one where a workgroup has the candidates; both kinds together are past one queue round of
        # the form that queued them all from 128 double survivors on
        assert g["want"]["tail_only"] == min(3 * n, 1250 - n)
        assert (g["want"]["tail_only"] + n > Q.FUSED_QCAP) == (n >= 129)


@pytest.mark.parametrize("ham", [False, True])
@pytest.mark.parametrize("m", Q.LENGTHS)
def test_which_strings_are_asked_about_their_first_window(m, ham):
    """lengths K2 - 1 .. K2 + 2: a string is asked again when it is longer than K2 — at K2 + 1 the substitutions and insertions, not the
    deletions; at K2 the insertions alone; strings shorter than K2 ask the table's filter about their last K characters"""
    g = Q.case("len%d_%s" % (m, "ham" if ham else "edit"))
    q = g["qs"][g["sat"][0]]
    kinds = {}
    for w in Q.flat_candidates(q, ham):
        tw, hw = Q.windows(w)
        kinds.setdefault(len(w) - m, set()).add((len(tw), hw is not None))
    assert set(kinds) == ({0} if ham else {-1, 0, 1})
    for dl, seen in kinds.items():
        assert seen == {(S.K2 if m + dl >= S.K2 else S.K, m + dl > S.K2)}, (m, dl, seen)


def test_one_lane_cases():
    both, tail = Q.case("lane_both"), Q.case("lane_tail")
    for g in (both, tail):
        s = g["qs"][g["sat"][2]]
        lane = Q.flat_candidates(s, False)[:8]
        assert len(set(lane)) == 8 and sorted(len(w) for w in lane) == [19, 20, 20, 20, 21, 21, 21, 21]     # position 1: all eight operations
        have = S.substrings(g["text"], S.K2)
        assert all(Q.windows(w)[0] in have for w in lane)
        assert all((Q.windows(w)[1] in have) == (g is both) for w in lane)
    assert tail["want"]["both"] == 0 and tail["want"]["tail_only"] >= 8 and both["want"]["both"] >= 8


def test_overflow_case_overflows_a_fresh_list_beside_entries_that_fail_the_first_window():
    w = Q.case("overflow257")["want"]
    assert w["occurring"] == Q.LCAP0 + 1 and w["tail_only"] > 0 and w["both"] > w["occurring"]
