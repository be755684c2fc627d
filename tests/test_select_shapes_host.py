"""tests/select_shapes.py reaches what each of its cases was built for — shown on the reference side alone: a census of every
(query, strand) group of every batch by brute force on the finished text (the set of all its substrings of a length), the reference's
neighbourhoods (oracle_lib.neighbors) and the layout arithmetic restated from hunt.hip; no GPU, no library under test."""
import pytest

import oracle_lib as O
import select_shapes as S
from conftest import revcomp

EXACT = ("occ_edit", "occ_ham", "lay_edit", "lay_ham", "ham2_i", "ham2_j1024", "ham2_j1025")
_subs = {}


def occurs(g, w):
    key = (g["name"], len(w))
    if key not in _subs:
        _subs[key] = S.substrings(g["text"], len(w))
    return w in _subs[key]


def census(g, s, hamming):
    """the distinct candidates of strand s that occur"""
    return {w for w in S.language(s, g["d"], hamming) if occurs(g, w)}


def kept(g, s, hamming):
    """the strings of the reference's neighbourhood of s that occur"""
    return {w for w in S.kept_set(s, g["d"], hamming) if occurs(g, w)}


def modes(name):
    g = S.genome(name)
    return [g["hamming"]] if "hamming" in g else [False, True]


@pytest.mark.parametrize("name", sorted(S.GENOMES))
def test_texts_are_small_and_plain(name):
    g = S.genome(name)
    assert len(g["text"]) <= 50_000 and set(g["text"]) == set(b"ACGT\n") and g["text"].endswith(b"\n")
    assert sum(g["seqlen"]) == len(g["text"]) and len(g["seqlen"]) == g["text"].count(b"\n") == 2
    assert all(len(b["qs"]) <= 300 for b in g["batches"].values())


def test_the_candidate_walk_agrees_with_the_reference():
    """candidates() restates the walk of neighbors.h; the reference's neighbourhood is its substring-minimal part (edit mode) or all of
    it (Hamming mode)"""
    occ = S.genome("occ_edit")["batches"]["d513"]
    for q in [occ["qs"][i] for i in occ["sat"][:2]] + list(S.LOW_QUERIES):
        for s in (q, revcomp(q)):
            lang, ref = S.language(s, 1, False), set(O.neighbors(s, 1, True))
            assert ref <= lang
            assert all(any(r in w for r in ref) for w in lang)                       # every candidate is kept or contains a kept one
            assert ref == {w for w in lang if not any(x != w and x in w for x in lang)}
            assert S.language(s, 1, True) == set(O.neighbors(s, 1, False))
    q = S.genome("ham2_i")["batches"][512]["qs"][3]
    assert S.language(q, 2, True) == set(O.neighbors(q, 2, False)) and len(S.language(q, 2, True)) == 1771
    q = S.genome("edit2")["batches"][400, "long2"]["qs"][3]
    lang = S.language(q, 2, False)
    assert S.kept_set(q, 2, False) == set(O.neighbors(q, 2, True)) <= lang           # (the hash-set form is the plain one)
    assert len(lang) < 10000


def test_the_flat_kernel_spells_every_string_once():
    """cand1's validity rule restated (select_shapes.flat_candidates): no two (position, operation) candidates of a strand are the
    same string, whatever the query — so the LDS list of k_search1s never holds duplicates and its length is the census of distinct
    occurring strings — and the candidates it leaves out of the reference's walk each contain one it keeps"""
    import random
    rng = random.Random(7)
    qs = list(S.LOW_QUERIES) + ["A" * 20, "AC" * 10, "AAC" * 7, "ACGT" * 5]
    qs += ["".join(rng.choices("AC", k=rng.randrange(13, 32))) for _ in range(300)] + ["".join(rng.choices("ACGT", k=rng.randrange(13, 32))) for _ in range(300)]
    for q in qs:
        for ham in (False, True):
            flat = S.flat_candidates(q, ham)
            assert len(flat) == len(set(flat)), q
            assert set(flat) <= S.language(q, 1, ham)
            assert all(any(f in w for f in flat) for w in S.language(q, 1, ham) - set(flat)), q
    # a proper prefix and its continuation by A's (the rank loop's tie) are never both kept: one contains the other
    for q in qs[:40]:
        ks = S.kept_set(q, 1, False)
        assert not any(a != b and a.startswith(b) for a in ks for b in ks)


@pytest.mark.parametrize("name", EXACT)
def test_every_group_holds_exactly_its_census(name):
    g = S.genome(name)
    ham = g["hamming"]
    for label, b in g["batches"].items():
        for i, q in enumerate(b["qs"]):
            for strand, s in enumerate((q, revcomp(q))):
                want = b["L"].get(2 * i + strand, 0)
                if i in b["sat"]:
                    got = census(g, s, ham)
                    assert len(got) == want, (name, label, i, strand)
                    if g["d"] == 1:
                        assert sum(1 for w in S.flat_candidates(s, ham) if occurs(g, w)) == want      # what l_n counts
                    if not ham:
                        # as many (position, operation) candidates as distinct strings: no equal neighbours, deletions and
                        # substitutions only, the query itself absent
                        assert all(a != c for a, c in zip(s, s[1:])) and all(len(w) <= len(s) for w in got) and not occurs(g, s)
                else:    # padding: none of the reference's strings occurs, so no candidate does
                    assert want == 0 and not kept(g, s, ham), (name, label, i, strand)
        assert b["leaves"] == sum(b["L"].values())


@pytest.mark.parametrize("name", ["occ_edit", "occ_ham"])
def test_occupancy_rows_fill_one_workgroup(name):
    g = S.genome(name)
    assert S.gpw_of(20, True) == S.gpw_of(20, False) == 12
    for label, n in (("a0", 0), ("a1", 1), ("b64", 64), ("b65", 65), ("c256", 256), ("c257", 257), ("d512", 512), ("d513", 513), ("e64", 64), ("e65", 65)):
        b = g["batches"][label]
        assert len(b["qs"]) == 24 and S.flat_cap(24) == 64
        for take in (True, False):
            assert S.per_workgroup(b, "L", take) == ({1: n} if n else {}), label
        assert 513 > 48 * 4                                                           # the census of d513 asks for the list of 512
    # the thresholds the rows stand on either side of
    assert (64, 256, 512) == (64, S.FUSED_LCAP // 2, S.FUSED_LCAP) and S.FUSED_QCAP == 512
    for label, n in (("e64", 64), ("e65", 65)):
        b = g["batches"][label]
        for grp, want in b["kept"].items():
            q = b["qs"][grp // 2]
            assert len(kept(g, revcomp(q) if grp & 1 else q, g["hamming"])) == want, (label, grp)
        assert S.per_workgroup(b, "kept", True) == {1: n} and b["leaves"] <= 256
    if not g["hamming"]:     # elsewhere in edit mode fewer strings are kept than occur: nsel differs from the list's length
        b = g["batches"]["d512"]
        nk = sum(len(kept(g, revcomp(b["qs"][grp // 2]) if grp & 1 else b["qs"][grp // 2], False)) for grp in b["L"])
        assert 64 < nk < 512


@pytest.mark.parametrize("name", ["lay_edit", "lay_ham"])
def test_layout_rows_sit_in_the_slots_they_name(name):
    g = S.genome(name)
    assert S.LAY_LENGTHS == (16, 17, 31, S.K + 1)
    for m, gpw_take, gpw_plain in ((16, 16, 16), (17, 14, 15), (31, 8, 8), (13, 16, 16)):
        b = g["batches"]["f%d" % m]
        assert {len(q) for q in b["qs"]} == {m}
        assert (S.gpw_of(m, True), S.gpw_of(m, False)) == (gpw_take, gpw_plain)
        lay = S.layout(b["qs"], True)
        first, second, last = b["sat"]
        assert second == first + 1 and len(b["qs"]) * 2 == 3 * gpw_take
        assert [lay[2 * first], lay[2 * first + 1], lay[2 * second]] == [(1, 0), (1, 1), (1, 2)]          # slot 0, and side by side
        assert [lay[2 * last], lay[2 * last + 1]] == [(1, gpw_take - 2), (1, gpw_take - 1)]               # the last slot
        assert S.per_workgroup(b, "L", True) == {1: 46}
        # all six censuses differ from their neighbours': strings that move between groups change the sums
        assert [b["L"][2 * i + s] for i in (first, second) for s in (0, 1)] == [9, 5, 7, 11]
    b = g["batches"]["f17"]                                                           # odd gpw: a query split across two workgroups
    lay = S.layout(b["qs"], False)
    first = b["sat"][0]
    assert [lay[2 * first], lay[2 * first + 1]] == [(0, 14), (1, 0)]
    assert S.per_workgroup(b, "L", False) == {0: 9, 1: 37}


def test_low_complexity_queries_have_everything_planted():
    g = S.genome("low")
    for ham in (False, True):
        b = g["batches"][ham]
        assert [S.layout(b["qs"], True)[2 * i] for i in b["sat"]] == [(0, 0), (1, 2), (2, 10)]          # a query per workgroup
        for i in b["sat"]:
            q = b["qs"][i]
            assert census(g, q, ham) == S.language(q, 1, ham) and occurs(g, q)
            assert len(census(g, revcomp(q), ham)) >= (9 if ham else 1)
            # no LDS list overflows: even with every duplicate of the reference's walk counted the workgroup stays below 256
            dup = sum(1 for s in (q, revcomp(q)) for w in S.candidates(s, 1, ham) if occurs(g, w))
            flat = sum(1 for s in (q, revcomp(q)) for w in S.flat_candidates(s, ham) if occurs(g, w))
            assert max(dup, flat) <= S.FUSED_LCAP // 2, (q, dup, flat)
            if not ham:   # most strings contain one another, equal strings come from several operations
                assert len(kept(g, q, False)) < len(S.language(q, 1, False)) < len(S.candidates(q, 1, False))
        for i, q in enumerate(b["qs"]):
            if i not in b["sat"]:
                assert not kept(g, q, ham) and not kept(g, revcomp(q), ham)
    q1 = S.LOW_QUERIES[1]
    q0 = S.LOW_QUERIES[0]
    assert len(set(S.dels(q0))) == 15 and len(S.dels(q0)) == 20                       # the run of six A: six deletions, one string


def test_long_queries_are_packed_or_not():
    g = S.genome("long")
    for ham in (False, True):
        for m in (41, 42):
            b = g["batches"][m, ham]
            (i,) = b["sat"]
            q = b["qs"][i]
            assert len(q) == m and (m + 1 <= S.PACK_MAX_LEN) == (m == 41)
            n = len(census(g, q, ham))
            assert sum(1 for w in S.dels(q) + S.subs(q) if occurs(g, w)) == 100 and 60 <= n <= 110, n   # (a spacer may spell an insertion)
            assert all(len(p) == 20 and not kept(g, p, ham) and not kept(g, revcomp(p), ham) for j, p in enumerate(b["qs"]) if j != i)


def test_edit_distance_two_is_bracketed():
    g = S.genome("edit2")
    assert len(g["short"]) == S.K2 + 1 >= S.K + 2
    for c in (513, 400):
        for body in ("long2", "r04"):
            b = g["batches"][c, body]
            q = b["qs"][3]
            assert len(q) == 16 >= S.K2 + 2 and len(kept(g, q, False)) == c and len(kept(g, revcomp(q), False)) == S.REV2
            for i, p in enumerate(b["qs"]):
                if i != 3:
                    assert not kept(g, p, False) and not kept(g, revcomp(p), False)
            assert (g["short"] in b["qs"]) == (body == "r04")
        lo, hi = S.bracket(g, b)
        print("edit2 %d: %d distinct occurring candidates, %d with the walk's duplicates" % (c, lo, hi))
        assert c + S.REV2 <= lo <= hi
        if c == 400:
            assert hi <= S.FUSED2_LCAP      # whatever repeated operations a kernel skips, the list holds the group
        else:
            assert lo > S.FUSED2_LCAP


@pytest.mark.parametrize("name", sorted(S.GENOMES))
def test_reference_sums_are_the_texts_own(name):
    """what the GPU test holds count mode against: per strand the occurrences of the kept strings, counted with bytes.find"""
    g = S.genome(name)
    ref = S.reference(name)
    for ham in modes(name):
        seen = set()
        for label, b in g["batches"].items():
            if isinstance(label, tuple) and label[-1] in (False, True) and label[-1] != ham or label in (False, True) and label != ham:
                continue
            for i in b["sat"]:
                q = b["qs"][i]
                if q in seen:
                    continue
                seen.add(q)
                want = tuple(sum(S.scan(g["text"], w.encode()) for w in S.kept_set(s, g["d"], ham)) for s in (q, revcomp(q)))
                assert ref.sums([q], g["d"], ham) == [want], (name, label, q)
                if b["L"].get(2 * i):
                    assert want[0] >= 1
