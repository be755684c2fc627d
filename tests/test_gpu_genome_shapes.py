"""The product library on texts of other shapes than conftest.make_genome's (tests/genome_shapes.py): one sequence, 512 / 513 / 3 000
sequences, empty records, no N at all, N as the most frequent symbol, a missing base, A/T tandem repeats, N runs of exactly 2 and 3,
all IUPAC letters, texts of 1 to 4 097 symbols and texts over every byte value.  Each shape is built once with the GPU builder and goes
through the builder, seam, hunt, search, mappability and binary checks against the oracle (validated on the same inputs without a GPU
by tests/test_genome_shapes_host.py) and against brute force.  Product library only, no DICEY_* switch."""
import ctypes as C
import gzip
import os
import subprocess
import time

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import dicey_amd
import genome_shapes as S
import mappability_ref as R
import oracle_lib as O
from conftest import revcomp
from test_gpu_cli import _oracle_json
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
needs_ref = pytest.mark.skipif(O.ref_libs() is None, reason="oracle/_ref (reference thal.h / json.hpp builds) not present")
HUNT_NAMES = [n for n in S.NAMES if S.is_dna(n)]
OPEN_FLAGS = [{}, {"compact": True, "pre5": False}, {"kmer_table": False}]


class _Oracle:
    """the oracle's index of one shape; hunt() remembers its answers, so that the same batch under other open flags is not enumerated twice"""

    def __init__(self, path):
        self.ix = O.Index(path)
        self.memo = {}

    def hunt(self, seqlen, names, qs, **kw):
        key = (tuple(qs), tuple(sorted(kw.items())))
        if key not in self.memo:
            self.memo[key] = self.ix.hunt(seqlen, names, qs, **kw)
        return self.memo[key]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> shape with "fm9" (written by dicey_amd.build_index, once), "ref" (the oracle's file) and "orc" """
    d = tmp_path_factory.mktemp("shapes")
    made = {}

    def get(name):
        if name not in made:
            g = dict(S.all_shapes()[name])
            g["fm9"], g["ref"] = str(d / (name + ".fm9")), str(d / (name + ".ref.fm9"))
            dicey_amd.build_index(g["text"], g["fm9"])
            O.build_fm9(g["text"], g["ref"])
            g["orc"] = _Oracle(g["ref"])
            made[name] = g
        return made[name]
    return get


@pytest.fixture(scope="module")
def opened(built):
    """name -> FmIndex with the default flags, kept open for the module"""
    ixs = {}

    def get(name):
        if name not in ixs:
            ixs[name] = dicey_amd.FmIndex(built(name)["fm9"])
        return ixs[name]
    yield get
    for ix in ixs.values():
        ix.close()


# ---- builder ----------------------------------------------------------------------------------------------------------------------

def _first_difference(a, b, rep):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    sec = next((s["name"] for s in rep.get("sections", []) if s["offset"] <= k < s["offset"] + s["bytes"]), "?")
    return "first difference at byte %d (section %s), sizes %d / %d" % (k, sec, len(a), len(b))


@pytest.mark.parametrize("name", S.NAMES)
def test_builder_writes_the_oracle_file(built, tmp_path, name):
    """dg_index_build and dg_index_build_device (the text handed over as a torch tensor in HBM: what bench.py builds with) against the
    oracle's writer, byte for byte; dg_fm9_check deep accepts the file"""
    g = built(name)
    want = open(g["ref"], "rb").read()
    got = open(g["fm9"], "rb").read()
    rep = dicey_amd.check_fm9(g["ref"])
    assert got == want, (name, _first_difference(got, want, rep))
    rep = dicey_amd.check_fm9(g["fm9"], deep=True)
    assert rep["ok"] is True and rep["rc"] == 0, (name, rep.get("error"))
    assert rep["n"] == len(g["text"]) + 1 and rep["sigma"] == len(set(g["text"])) + 1
    from dicey_amd import _capi
    L = _capi.load()
    d_text = torch.frombuffer(bytearray(g["text"]), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    path = str(tmp_path / "device.fm9")
    _capi.check(L, L.dg_index_build_device(C.c_void_p(d_text.data_ptr()), len(g["text"]), 0, path.encode()))
    dev = open(path, "rb").read()
    assert dev == want, (name, _first_difference(dev, want, rep))


# ---- seam -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_count_locate_extract_match_brute_force(built, name):
    g = built(name)
    text = g["text"]
    pats = S.seam_patterns(name, g)
    want = [O.bf_locate(text, p) for p in pats]
    full = text + b"\0"
    rs = S.extract_ranges(name, g)
    for flags in OPEN_FLAGS:
        with dicey_amd.FmIndex(g["fm9"], **flags) as ix:
            cnt = ix.count(pats)
            loc = ix.locate(pats)
            ext = ix.extract(rs)
        for p, c, l, w in zip(pats, cnt, loc, want):
            assert c == len(w) and l == w, (name, flags, p, c, len(w), l[:5], w[:5])
        for (a, b), e in zip(rs, ext):
            assert e == full[a:b + 1], (name, flags, a, b)
    assert sum(1 for w in want if w) >= min(60, len(text))


# ---- hunt -------------------------------------------------------------------------------------------------------------------------

def _key(batch):
    return [[(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in q.hits] + [q.flags, q.nondna, q.sequence, q.distance]
            for q in batch.queries]


def _hit_floor(g, qs):
    """queries that are written in a sequence, letter for letter, and are made of A/C/G/T: every mode answers each of them with at least
    one hit (the occurrence itself is in every neighbourhood; max_locations = 3 still leaves one), so their number is a floor that owes
    nothing to the code under test"""
    t = g["text"].decode()
    return sum(1 for q in qs if len(q) >= 10 and set(q) <= set("ACGT") and q in t)


def _report(ix, g, name, mode, qs, kw):
    """after a mismatch: shape, mode, query and both hit lists of the first query that differs"""
    got = ix.hunt(qs, g["seqlen"], **kw)
    _, hits = g["orc"].hunt(g["seqlen"], g["names"], qs, want_hits=True, **kw)
    per = {}
    for h in hits:
        per.setdefault(h[0], []).append(h[1:])
    for qi, qr in enumerate(got.queries):
        a = [(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in qr.hits]
        if a != per.get(qi, []):
            print("MISMATCH shape %s mode %s query %d %r\n  library: %r\n  oracle:  %r" % (name, mode, qi, qs[qi], a, per.get(qi, [])))
            return


def _hunt_mode(ix, g, name, mode, tag=""):
    key, kw, lens, share = next(m for m in S.MODES if m[0] == mode)
    qs = S.hunt_queries(name, g, mode)
    if mode == "edit2":
        O.fast_neighbors(True)
    try:
        got = _compare(ix, g["orc"], g, qs, **kw)
    except AssertionError:
        _report(ix, g, name, mode, qs, kw)
        raise
    finally:
        O.fast_neighbors(False)
    nhits = sum(len(q.hits) for q in got.queries)
    above = sum(1 for q in got.queries for h in q.hits if h.chr >= 512)
    floor = _hit_floor(g, qs)
    print("hunt %s%s %s: %d queries, %d hits compared (floor %d), %d with chr >= 512" % (name, tag, mode, len(qs), nhits, floor, above))
    assert nhits >= floor, (name, mode, nhits, floor)
    if len(g["text"]) >= 500:
        assert floor >= 3, (name, mode, floor)      # the batch is not vacuous: it holds queries that must be found
    if len(g["seqs"]) > 512:
        assert above >= 50, (name, mode, above)
    return qs, kw, got


@pytest.mark.parametrize("mode", [m[0] for m in S.MODES])
@pytest.mark.parametrize("name", HUNT_NAMES)
def test_hunt_hits_equal_oracle_push_order(built, opened, name, mode):
    """every hit in push order with both alignment rows (_compare of test_gpu_parity.py); then the same batch delivered in the classic
    form and in the compact form followed by dg_hunt_expand must be the same result"""
    g = built(name)
    ix = opened(name)
    qs, kw, got = _hunt_mode(ix, g, name, mode)
    classic = ix.hunt(qs, g["seqlen"], compact=False, **kw)
    compact = ix.hunt(qs, g["seqlen"], compact=True, **kw)      # DG_HUNT_COMPACT, expanded by dg_hunt_expand in FmIndex._unpack
    assert _key(compact) == _key(classic), (name, mode)
    assert _key(got) == _key(classic), (name, mode)


@pytest.mark.parametrize("name", HUNT_NAMES)
def test_hunt_with_the_one_shot_open_flags(built, name):
    """DG_OPEN_COMPACT | DG_OPEN_NO_PRE5, what `dicey hunt` opens a single input with: every mode again"""
    g = built(name)
    with dicey_amd.FmIndex(g["fm9"], compact=True, pre5=False) as ix:
        for m in S.MODES:
            _hunt_mode(ix, g, name, m[0], tag=" (one-shot flags)")


def test_code_lengths_follow_the_symbol_frequencies(built, opened):
    """the Huffman shapes the issue names, read from dg_index_stats: N holds the shortest code on the hard-masked text, C has none on the
    bisulfite text, A/T take one or two bits on the tandem text, 17 symbols on the IUPAC text"""
    out = {}
    for name in ("hard_masked", "bisulfite", "at_tandem", "iupac_rich", "single_no_n"):
        st = opened(name).stats()
        cl = {chr(b): v for b, v in st["code_len"].items() if b}
        out[name] = (st["sigma"], cl)
        orc = built(name)["orc"].ix
        assert all(cl.get(c, 0) == orc.code_len(c) for c in "ACGTN\n" + S.AMBIG), (name, cl)
        print("codes %s: sigma %d, N %d, A %d, C %d, G %d, T %d" % (name, st["sigma"], cl.get("N", 0), cl.get("A", 0), cl.get("C", 0),
                                                                     cl.get("G", 0), cl.get("T", 0)))
    sig, cl = out["hard_masked"]
    assert sig == 7 and cl["N"] < min(cl[c] for c in "ACGT")
    sig, cl = out["bisulfite"]
    assert sig == 6 and "C" not in cl
    sig, cl = out["at_tandem"]
    assert sig == 4 and set(cl) == {"A", "T", "\n"}
    sig, cl = out["iupac_rich"]
    assert sig == 17 and len(cl) == 16
    sig, cl = out["single_no_n"]
    assert sig == 6 and "N" not in cl


# ---- search -----------------------------------------------------------------------------------------------------------------------

def _primers(name, g):
    """primers of 18-24 nt cut from the text, some with one mismatch; for the many-sequence shapes most of them from sequences above
    index 512, with their last 15 nt (the k-mer that is searched) within 30 nt of the start or the end of the sequence"""
    import random
    rng = random.Random(S.hash_name(name) + 9)
    seqs = g["seqs"]
    out = []
    pool = [i for i, s in enumerate(seqs) if len(s) >= 60 and (len(seqs) == 1 or i >= 512)]
    while len(out) < 16:
        i = rng.choice(pool)
        s = seqs[i]
        m = rng.randint(18, 24)
        where = len(out) % 4
        a = rng.randrange(0, 6) if where == 0 else (len(s) - m - rng.randrange(0, 6) if where == 1 else rng.randrange(len(s) - m + 1))
        p = s[a:a + m]
        if set(p) - set("ACGT"):
            continue
        if where == 3:
            p = revcomp(p)
        if len(out) % 5 == 4:
            k = rng.randrange(0, m - 15)        # outside the 15 nt that are searched
            p = p[:k] + rng.choice("ACGT") + p[k + 1:]
        out.append(p)
    if len(seqs) > 512:   # and the two sides of the edge below it: the first sequence that has 20 nt, and sequence 511
        first = next(s for s in seqs if len(s) >= 20)
        out += [p for p in (first[:20], seqs[511][-20:]) if len(p) == 20 and not set(p) - set("ACGT")]
    return out


@needs_ref
@pytest.mark.parametrize("name", ["many_short", "seq513", "single_no_n"])
def test_search_sites_equal_the_oracle_search(built, opened, name):
    import json
    g = built(name)
    prim = _primers(name, g)
    fasta = "".join(">p%d\n%s\n" % (i, p) for i, p in enumerate(prim))
    want, rc = g["orc"].ix.search(g["seqlen"], g["names"], g["text"], fasta)
    assert rc == 0, want[:300]
    doc = json.loads(want)
    ref_of = {n: i for i, n in enumerate(g["names"])}
    exp = sorted((ref_of[p["Chrom"]], p["Pos"] - 1, int(p["Name"][1:]), p["Ori"] == "forward", p["Tm"], p["MatchTm"], p["Genome"])
                 for p in doc["data"]["primers"])
    th = dicey_amd.Thal(O.PRIMER3_CONFIG)
    try:
        sites, mt, fl, nh = dicey_amd.search_sites(opened(name), th, prim, g["seqlen"])
    finally:
        th.close()
    got = sorted((s["ref"], s["pos"], s["primer"], s["on_for"], s["temp"], s["perf_temp"], s["genome"]) for s in sites)
    assert got == exp, (name, [x for x in got if x not in exp][:3], [x for x in exp if x not in got][:3])
    assert len(got) >= 12
    if len(g["seqs"]) > 512:   # binding sites above sequence 512 whose k-mer lies within 30 nt of a sequence end
        near = [s for s in got if s[0] >= 512 and (s[1] < 30 or s[1] + 30 > g["seqlen"][s[0]] - 1 - 15)]
        print("search %s: %d sites, %d above sequence 512 and next to a sequence end" % (name, len(got), len(near)))
        assert len(near) >= 6


# ---- mappability ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["many_short", "hard_masked", "at_tandem", "single_no_n"])
def test_mappability_equals_the_brute_force_count(built, opened, name):
    g = built(name)
    text = g["text"]
    ix = opened(name)
    for k in (10, 20, 32):
        got = ix.mappability(k=k)
        exp = R.values(text, k)
        assert len(got) == len(text)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (name, k, bad[:10], got[bad[:10]], exp[bad[:10]])
        assert exp.any()
    if name == "many_short":   # runs over ranges that start inside an empty record (its '\n'), at the adjacent pair and at the first byte
        t = text
        vals = R.values(text, 20)
        starts = [0] + [i for i in range(1, len(t)) if t[i] == 10 and t[i - 1] == 10][:8]
        assert len(starts) >= 6
        for lo in starts:
            for hi in (lo + 1, lo + 700, len(t)):
                got = ix.mappability_runs(k=20, lo=lo, hi=min(hi, len(t)))
                ref = R.runs(vals, lo, min(hi, len(t)))
                for x, y in zip(got, ref):
                    assert (x == y).all(), (lo, hi)


# ---- binary -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many_short_fasta(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("shapes_cli")
    g = dict(S.all_shapes()["many_short"])
    fa = d / "contigs.fa.gz"
    with gzip.open(fa, "wt", compresslevel=1) as f:
        for i, (n, s) in enumerate(zip(g["names"], g["seqs"])):
            f.write(">%s%s\n" % (n, " len=%d" % len(s) if i % 3 == 0 else ""))   # an empty record is its header line alone
            for a in range(0, len(s), 60):
                f.write(s[a:a + 60] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g.update(fa=str(fa), fm9=str(d / "contigs.fa.fm9"), dir=d)
    return g


def test_binary_index_and_hunt_on_three_thousand_records(many_short_fasta):
    """`dicey index` writes the oracle's file for a FASTA with empty records (adjacent separators, src/index.h:105-113), and `dicey hunt`
    names 3 000 records like the oracle: JSON byte for byte"""
    g = many_short_fasta
    ref = str(g["dir"] / "oracle.fm9")
    O.build_fm9(g["text"], ref)
    assert open(g["fm9"], "rb").read() == open(ref, "rb").read()
    qs = S.hunt_queries("many_short", g, "edit1")
    names = ["q%d" % i for i in range(len(qs))]
    qf = g["dir"] / "queries.fa"
    with open(qf, "w") as f:
        for n, s in zip(names, qs):
            f.write(">%s\n%s\n" % (n, s))
    want = _oracle_json(g, qs, names, distance=1)
    r = subprocess.run([DICEY, "hunt", "-g", g["fa"], str(qf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    if r.stdout != want:
        a, b = r.stdout.split("\n"), want.split("\n")
        k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        print("MISMATCH query %d %r\n  binary: %s\n  oracle: %s" % (k, qs[k] if k < len(qs) else None, a[k:k + 1], b[k:k + 1]))
    assert r.stdout == want
    import json
    above = sum(1 for ln in r.stdout.split("\n") if ln for h in json.loads(ln).get("data", []) if int(h["chr"][3:]) > 512)
    assert above >= 50, above       # names of records above index 512, as the oracle writes them


def test_binary_mappability_on_three_thousand_records(many_short_fasta):
    """`dicey mappability`: the bedGraph cut per sequence; empty sequences and sequences shorter than k produce no line.  Then the names
    of a .fai take the place of the FASTA's"""
    g = many_short_fasta
    for k in (20, 32):
        exp = R.bedgraph(g["text"], g["names"], k)
        r = subprocess.run([DICEY, "mappability", "-g", g["fa"], "-k", str(k)], capture_output=True)
        assert r.returncode == 0, r.stderr[-1500:]
        assert r.stdout == exp
        seen = {ln.split(b"\t")[0].decode() for ln in r.stdout.split(b"\n") if ln}
        silent = {n for n, s in zip(g["names"], g["seqs"]) if len(s) < k}
        assert len(silent) >= 300 and not (seen & silent) and len(seen) >= 2000
    with open(g["fa"] + ".fai", "w") as f:
        for i, s in enumerate(g["seqs"]):
            f.write("n%d\t%d\t%d\t%d\t%d\n" % (i, len(s), 0, 60, 61))
    try:
        r = subprocess.run([DICEY, "mappability", "-g", g["fa"], "-k", "20", "-f"], capture_output=True)
        assert r.returncode == 0, r.stderr[-1500:]
        assert r.stdout == R.bedgraph(g["text"], ["n%d" % i for i in range(len(g["seqs"]))], 20, forward_only=True)
    finally:
        os.remove(g["fa"] + ".fai")
