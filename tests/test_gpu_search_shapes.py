"""The site stage of `dicey search` (k_site_wave, k_site, k_site_keep / k_site_compact and the host loop of dg_search_sites) on the
cases of tests/search_shapes.py, against the oracle: sites in the reference's push order with Tm as doubles bit for bit, MatchTm,
flags and the located-hit count at library level; the product library, the development build under each of its three site-stage
switches (one fresh child process per switch), the binary byte for byte, and two batches in both orders on one handle."""
import gzip
import os
import pickle
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # the child processes below start this file as a script
    sys.path.insert(0, ROOT)

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import dicey_amd
import oracle_lib as O
import search_shapes as S
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
DG_P_THAL_FAILED = 16      # include/dicey_gpu.h; dicey_amd/_capi.py mirrors neither this flag nor the error codes
DG_ELIMIT = -7
SWITCHES = ["DICEY_NO_WAVE_THAL", "DICEY_NO_LDS_TABLES", "DICEY_DEBUG_THAL_REDO"]     # every case runs under each of them


def _want(e):
    return {"pushed": [p[:4] + (S.bits(p[4]), S.bits(p[5]), p[6]) for p in e["pushed"]],
            "match_temp": None if e["match_temp"] is None else [S.bits(t) for t in e["match_temp"]],
            "max_matches": e["max_matches"], "nbhd_warnings": e["nbhd_warnings"], "nhits": len(e["located"]), "primers": e["primers"]}


def compare(ix, th, seqlen, want, kw, tag):
    """one batch through dg_search_sites against what the oracle pushed, in order"""
    sites, mt, fl, nh = dicey_amd.search_sites(ix, th, want["primers"], seqlen, **kw)
    got = [(s["ref"], s["pos"], s["primer"], s["on_for"], S.bits(s["temp"]), S.bits(s["perf_temp"]), s["genome"]) for s in sites]
    exp = want["pushed"]
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        print("MISMATCH %s at site %d of %d / %d\n  library: %r\n  oracle:  %r" % (tag, k, len(got), len(exp), got[k:k + 2], exp[k:k + 2]))
    assert got == exp, tag
    if want["match_temp"] is not None:
        assert [S.bits(t) for t in mt] == want["match_temp"], tag
    assert [bool(f & _capi.DG_Q_MAX_MATCHES) for f in fl] == want["max_matches"], tag
    assert sum(1 for f in fl if f & _capi.DG_Q_NBHD_EXCEEDED) == want["nbhd_warnings"], tag
    assert not any(f & DG_P_THAL_FAILED for f in fl), tag
    assert nh == want["nhits"], (tag, nh, want["nhits"])
    return len(got)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """the text as genome.fa.gz with the GPU builder's index next to it, where the binary looks for it"""
    assert O.ref_libs() is not None, "oracle/_ref is missing: __graft_entry__.build() compiles it (oracle/Makefile)"
    g = dict(S.genome())
    d = tmp_path_factory.mktemp("search_shapes")
    fa = d / "genome.fa.gz"
    with gzip.open(fa, "wt", compresslevel=1) as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">%s\n" % n)
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + "\n")
    g.update(dir=d, fa=str(fa), fm9=str(d / "genome.fa.fm9"))
    dicey_amd.build_index(g["text"], g["fm9"])
    return g


@pytest.fixture(scope="module")
def handles(shapes):
    ix = dicey_amd.FmIndex(shapes["fm9"])
    th = dicey_amd.Thal(O.PRIMER3_CONFIG)
    yield ix, th
    th.close()
    ix.close()


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_product_library_pushes_the_oracle_sites_in_order(shapes, handles, name):
    ix, th = handles
    case = S.cases()[name]
    n = compare(ix, th, shapes["seqlen"], _want(S.expected(name)), S.library_kw(case), name)
    print("%s: %d sites equal, in order" % (name, n))


def test_cut_on_below_and_above_a_site_tm(shapes, handles):
    """cut_temp equal to a site's Tm drops that site, the next double below keeps it: `> cut` is strict on the device and on the host"""
    from test_search_shapes_host import cut_values
    ix, th = handles
    case = S.cases()["cut_edge"]
    for c in cut_values():
        compare(ix, th, shapes["seqlen"], _want(S.expected("cut_edge", cutTemp=c)), S.library_kw(case, cutTemp=c), "cut_edge %r" % c)


def test_refused_primers_set_their_flag_and_leave_the_others_alone(shapes, handles):
    """a 61-nt and a 64-nt primer: thal() takes neither against its complement nor against a window over 60 nt -> DG_P_THAL_FAILED and
    no site; the 20-mers around them keep the sites the oracle gives them alone.  65 nt: DG_ELIMIT"""
    ix, th = handles
    r = S.refused_primers()
    base = S.cases()["refused_base"]
    e = S.expected("refused_base")
    prim = [e["primers"][0], r["p61"], e["primers"][1], r["p64"], e["primers"][2]]
    where = {0: 0, 1: 2, 2: 4}
    sites, mt, fl, nh = dicey_amd.search_sites(ix, th, prim, shapes["seqlen"], **S.library_kw(base))
    got = [(s["ref"], s["pos"], s["primer"], s["on_for"], S.bits(s["temp"]), S.bits(s["perf_temp"]), s["genome"]) for s in sites]
    assert got == [(p[0], p[1], where[p[2]], p[3], S.bits(p[4]), S.bits(p[5]), p[6]) for p in e["pushed"]]
    assert [bool(f & DG_P_THAL_FAILED) for f in fl] == [False, True, False, True, False]
    assert mt[1] == mt[3] == -999999.0      # thal()'s -infinity (thal.h _INFINITY)
    # each refused primer was cut from the text: its 15-mer is located wherever the text holds it or a neighbour at edit distance 1
    # (counted by the oracle on their last 20 nt: what is located depends on the searched 15-mer alone)
    tails = [r["p61"][-20:], r["p64"][-20:]]
    loc = S.oracle_index().search(shapes["seqlen"], shapes["names"], shapes["text"], S.fasta(tails), want_log=True, **S.oracle_kw(base))[2]
    own = [sum(1 for h in loc if h[0] == i) for i in range(2)]
    assert min(own) >= 1 and nh == len(e["located"]) + sum(own), (nh, len(e["located"]), own)
    with pytest.raises(dicey_amd.DgError) as err:
        dicey_amd.search_sites(ix, th, prim[:2] + [r["p65"]], shapes["seqlen"], **S.library_kw(base))
    assert err.value.code == DG_ELIMIT
    compare(ix, th, shapes["seqlen"], _want(e), S.library_kw(base), "refused_base after DG_ELIMIT")   # the handle is still good


def test_results_do_not_depend_on_what_the_handle_did_before(shapes):
    """a batch of 20-mers after a batch of 58-60-mers and the reverse, on one handle each: workspaces and the wave kernel's LDS size
    are reused"""
    orders = [["sequential_58_60_d1", "refused_base", "trace2600", "len31_57", "cut_edge"],
              ["cut_edge", "len31_57", "trace2600", "refused_base", "sequential_58_60_d1", "cut_edge"]]
    for order in orders:
        with dicey_amd.FmIndex(shapes["fm9"]) as ix:
            th = dicey_amd.Thal(O.PRIMER3_CONFIG)
            try:
                for name in order:
                    compare(ix, th, shapes["seqlen"], _want(S.expected(name)), S.library_kw(S.cases()[name]), "%s in %s" % (name, order))
            finally:
                th.close()


# ---- the development build, one switch per fresh process -------------------------------------------------------------------------------

def _child(fm9, blob):
    """runs in a child whose environment holds one DICEY_* switch: conftest.open_index then opens the development build"""
    from conftest import exp_lib, open_index
    jobs, seqlen = pickle.load(open(blob, "rb"))
    with open_index(fm9) as ix:
        assert ix._L is exp_lib()
        th = dicey_amd.Thal(O.PRIMER3_CONFIG, _lib=exp_lib())
        try:
            for name, want, kw in jobs:
                n = compare(ix, th, seqlen, want, kw, name)
                print("%s: %d sites equal" % (name, n), flush=True)
        finally:
            th.close()


def test_development_build_under_each_site_stage_switch(shapes):
    from conftest import build_exp_lib
    build_exp_lib()
    names = S.CASE_NAMES
    for switch in SWITCHES:      # one at a time; the first failure stops the rest
        blob = str(shapes["dir"] / (switch + ".pickle"))
        jobs = [(n, _want(S.expected(n)), S.library_kw(S.cases()[n])) for n in names]
        pickle.dump((jobs, shapes["seqlen"]), open(blob, "wb"))
        env = dict(os.environ)
        env[switch] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shapes["fm9"], blob], env=env, capture_output=True,
                           text=True, timeout=180)
        print(switch, r.stdout.replace("\n", "; "))
        assert r.returncode == 0, (switch, r.stdout[-1500:], r.stderr[-1500:])
        assert r.stdout.count("sites equal") == len(names), (switch, r.stdout)


# ---- the binary ------------------------------------------------------------------------------------------------------------------------

def _flags(case):
    a = ["-k", str(case["kmer"]), "-d", str(case["distance"]), "-c", repr(case["cutTemp"])]
    if case["hamming"]:
        a.append("-n")
    if "maxNeighborhood" in case:
        a += ["-x", str(case["maxNeighborhood"])]
    return a


def _binary(shapes, tag, primers, case):
    pf = shapes["dir"] / (tag + ".fa")
    pf.write_text(S.fasta(primers))
    want, wrc = S.oracle_index().search(shapes["seqlen"], shapes["names"], shapes["text"], S.fasta(primers), genome=shapes["fa"],
                                        **S.oracle_kw(case))
    r = subprocess.run([DICEY, "search", "-i", O.PRIMER3_CONFIG, "-g", shapes["fa"], *_flags(case), str(pf)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == wrc, (tag, r.returncode, wrc, r.stderr[-800:])
    if r.stdout != want:
        k = next((i for i in range(min(len(r.stdout), len(want))) if r.stdout[i] != want[i]), min(len(r.stdout), len(want)))
        print("MISMATCH %s at byte %d\n  binary: %r\n  oracle: %r" % (tag, k, r.stdout[max(0, k - 100):k + 100], want[max(0, k - 100):k + 100]))
    assert r.stdout == want, tag
    return wrc


@pytest.mark.parametrize("name", ["len31_57", "distance2_edit_k13", "distance2_hamming_k15", "dirty_windows", "palindromes", "trace2600"])
def test_binary_json_is_the_oracle_json(shapes, name):
    case = S.cases()[name]
    assert _binary(shapes, name, case["primers"], case) == 0


@pytest.mark.parametrize("key", ["p61", "p64", "p65"])
def test_binary_answers_a_refused_primer_with_the_error_json(shapes, key):
    """the reference ends at the first primer thal() refuses with "Error: Thermodynamical calculation failed!" and exit code 1, the
    warnings of the primers before it ahead of the error; a 65-nt primer is no different from a 61-nt one"""
    base = S.cases()["refused_base"]
    prim = ["ACGTNACGTRACGTACGTACGT"] + base["primers"][:2] + [S.refused_primers()[key]] + base["primers"][2:]
    assert _binary(shapes, "refused_" + key, prim, base) == 1


def test_randomised_wide_search_configurations_against_oracle():
    """tools/fuzz_search.py in its wide mode: primers of 16-60 nt, k 10-30, distance 0-2, -x"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_search.py"), "12", "10", "wide"], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "failing configurations: 0" in r.stdout, r.stdout[-1500:]


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "--child":
    _child(sys.argv[2], sys.argv[3])
