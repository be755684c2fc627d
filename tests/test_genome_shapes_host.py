"""The reference side of tests/test_gpu_genome_shapes.py, validated without a GPU: for every shape of tests/genome_shapes.py the
oracle's index file passes the product's deep file check, its suffix array equals a naive suffix sort written here (which knows nothing
of sdsl), its count / locate / extract equal a brute-force scan on the very patterns the GPU module runs, and the shapes that exist to
reach one code path assert the property that reaches it."""
from collections import Counter

import pytest

import genome_shapes as S
import oracle_lib as O


@pytest.fixture(scope="module")
def oracle_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("shapes_host")
    made = {}

    def get(name):
        if name not in made:
            path = str(d / (name + ".fm9"))
            O.build_fm9(S.all_shapes()[name]["text"], path)
            made[name] = path
        return made[name]
    return get


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_file_passes_the_deep_check(oracle_file, name):
    import dicey_amd
    rep = dicey_amd.check_fm9(oracle_file(name), deep=True)
    assert rep["ok"] is True and rep["rc"] == 0, (name, rep.get("error"))
    text = S.all_shapes()[name]["text"]
    assert rep["n"] == len(text) + 1 and rep["sigma"] == len(set(text)) + 1


def naive_suffix_array(t):
    """suffixes of t (bytes, ending with the unique smallest byte 0) in lexicographic order, by comparing the suffixes themselves"""
    return sorted(range(len(t)), key=lambda i: t[i:])


@pytest.mark.parametrize("name", [n for n in S.NAMES if len(S.all_shapes()[n]["text"]) <= 20000])
def test_oracle_suffix_array_equals_a_naive_suffix_sort(oracle_file, name):
    t = S.all_shapes()[name]["text"] + b"\0"
    ix = O.Index(oracle_file(name))
    assert ix.size == len(t)
    want = naive_suffix_array(t)
    got = [ix.sa(i) for i in range(len(t))]
    assert got == want, (name, next(i for i in range(len(t)) if got[i] != want[i]))


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_count_locate_extract_equal_brute_force(oracle_file, name):
    g = S.all_shapes()[name]
    text = g["text"]
    ix = O.Index(oracle_file(name))
    pats = S.seam_patterns(name, g)
    assert len(pats) >= 150 and any(len(p) > len(text) for p in pats) and any(b"\n" in p[1:-1] for p in pats if len(p) > 2) or len(text) < 3
    found = 0
    for p in pats:
        want = O.bf_locate(text, p)
        assert ix.count(p) == len(want), (name, p)
        assert sorted(ix.locate(p)) == want, (name, p)
        found += bool(want)
    assert found >= min(60, len(text)), (name, found)
    full = text + b"\0"
    for a, b in S.extract_ranges(name, g):
        assert ix.extract(a, b) == full[a:b + 1], (name, a, b)


def _lengths(name):
    return [len(s) for s in S.all_shapes()[name]["seqs"]]


@pytest.mark.parametrize("r", [2, 3])
def test_nrun_shapes_have_runs_of_one_length_only(r):
    g = S.all_shapes()["nrun%d" % r]
    assert S.n_run_lengths(g["text"]) == {r}
    assert g["text"].count(b"N") >= 150 * r
    s = g["seqs"]
    assert s[0].startswith("N" * r) and s[0].endswith("N" * r)          # a run at either end of a sequence
    assert s[1][1:1 + r] == "N" * r and s[1][0] != "N" and s[2][2:2 + r] == "N" * r and s[2][1] != "N"   # and 1 and 2 letters inside


def test_sequence_counts_sit_on_both_sides_of_the_lds_edge():
    a, b = S.all_shapes()["seq512"], S.all_shapes()["seq513"]
    assert len(a["seqlen"]) == len(a["seqs"]) == 512 and len(b["seqlen"]) == len(b["seqs"]) == 513
    for g in (a, b):
        assert all(60 <= len(s) <= 150 for s in g["seqs"])
        assert g["text"].count(b"\n") == len(g["seqs"])
    assert len(b["seqs"][512]) == 150


def test_many_short_has_its_empty_and_short_records():
    L = _lengths("many_short")
    g = S.all_shapes()["many_short"]
    assert len(L) == 3000 and 350000 <= len(g["text"]) <= 450000
    empty = [i for i, m in enumerate(L) if m == 0]
    assert len(empty) == 8 and empty == list(S.MANY_SHORT_EMPTY)
    assert any(b - a == 1 for a, b in zip(empty, empty[1:]))              # two adjacent: three '\n' in a row
    assert b"\n\n\n" in g["text"] and g["text"].startswith(b"\n") and g["text"].endswith(b"\n\n")
    assert sum(1 for m in L if 0 < m < 20) >= 300 and max(L) <= 400        # the issue asks for at least 100
    assert L[1201] == 12 and L[1200] >= 20 and L[1202] >= 20
    assert sum(1 for m in L[512:] if m >= 31) >= 1500                     # most of the text lies above sequence 512
    assert 0 < g["text"].count(b"N") < len(g["text"]) // 50


def test_texts_that_lack_a_letter():
    A = S.all_shapes()
    assert len(A["single_no_n"]["seqs"]) == 1 and set(A["single_no_n"]["text"]) == set(b"ACGT\n")
    assert S.n_run_lengths(A["single_no_n"]["text"]) == set() and len(A["single_no_n"]["text"]) == 300001
    assert set(A["bisulfite"]["text"]) == set(b"AGTN\n") and len(A["bisulfite"]["seqs"]) == 3
    assert set(A["at_tandem"]["text"]) == set(b"AT\n")


def test_hard_masked_is_mostly_n_in_long_runs(oracle_file):
    g = S.all_shapes()["hard_masked"]
    text = g["text"]
    assert len(g["seqs"]) == 4
    for s in g["seqs"]:
        assert 0.55 <= s.count("N") / len(s) <= 0.65
    runs = S.n_run_lengths(text)
    assert min(runs) == 50 and max(runs) <= 5000
    cnt = Counter(text)
    assert cnt.most_common(1)[0][0] == ord("N")
    ix = O.Index(oracle_file("hard_masked"))
    assert ix.code_len("N") == min(ix.code_len(c) for c in "ACGTN\n") and ix.code_len("N") < min(ix.code_len(c) for c in "ACGT")


def test_absent_letters_have_no_code(oracle_file):
    assert O.Index(oracle_file("bisulfite")).code_len("C") == 0
    assert O.Index(oracle_file("single_no_n")).code_len("N") == 0
    ix = O.Index(oracle_file("at_tandem"))
    assert [ix.code_len(c) for c in "CGN"] == [0, 0, 0] and ix.code_len("A") >= 1 and ix.code_len("T") >= 1


def test_at_tandem_has_long_tandem_repeats():
    g = S.all_shapes()["at_tandem"]
    s = g["seqs"][0]
    period = next(p for p in range(1, 8) if s[:20000] == s[p:20000 + p])
    assert 1 <= period <= 7                                                # a tandem repeat of more than 20 kb at the start
    kmers = Counter(s[i:i + 20] for i in range(len(s) - 19))
    assert kmers.most_common(1)[0][1] >= 3000 and sum(1 for v in kmers.values() if v == 1) >= 200   # huge intervals and unique islands


def test_iupac_rich_has_every_letter_and_ties():
    g = S.all_shapes()["iupac_rich"]
    cnt = Counter(g["text"].decode())
    assert set(cnt) == set("ACGT" + S.AMBIG + "\n")
    n = len(g["text"])
    for c in S.AMBIG:
        assert 0.01 <= cnt[c] / n <= 0.05, (c, cnt[c])
    ties = Counter(cnt[c] for c in S.AMBIG)
    assert ties.most_common(1)[0][1] >= 3                                 # at least three letters with exactly the same count


def test_tiny_texts_have_the_listed_sizes():
    A = S.all_shapes()
    assert A["tiny_1"]["text"] == b"\n" and A["tiny_2a"]["text"] == b"A\n" and A["tiny_2n"]["text"] == b"\n\n"
    assert [len(A["tiny_%d" % n]["text"]) for n in S.TINY_SIZES] == list(S.TINY_SIZES)
    assert set(S.TINY_SIZES) >= {5, 62, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097}


def test_bytes_wide_covers_the_byte_values():
    A = S.all_shapes()
    assert set(A["bytes_wide"]["text"]) == set(range(1, 256)) and len(A["bytes_wide"]["text"]) == 20000
    assert len(set(A["bytes_w70"]["text"])) == 70 and len(A["bytes_w70"]["text"]) == 20000
    for name in S.BYTES_NAMES:
        g = A[name]
        assert b"\n".join(g["seqs"]) + b"\n" == g["text"] and g["seqlen"] == [len(s) + 1 for s in g["seqs"]]
