"""Every thal kernel of the product library against the reference's own thal() (oracle/_ref/libthalref.so, the unmodified
thal.h), bit for bit, on the generated corpus of thal_corpus.py and on generated padlock / search inputs:

  k_thal_wave, k_thal           dg_thal_batch, one batch per corpus group (the wave kernel's LDS layout follows the batch maxima),
                                then every group in one shuffled batch
  k_thal_self_wave<false|true>  dg_padlock_scan: arm and probe windows against their reverse complements
  k_site_wave, k_site           dg_search_sites: a primer against the context window of each hit

No test switches: everything runs on the product library."""
import os
import random
import struct

import pytest

import oracle_lib as O
import thal_corpus as TC
import thal_expect as TE
from conftest import make_genome, genome_text, revcomp

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not TE.have_ref(), reason="oracle/_ref (the reference's thal.h built in place) is not available")]


def _thal(env):
    import dicey_amd
    return dicey_amd.Thal(O.PRIMER3_CONFIG, **TC.ENVS[env])


def _tm(th, pairs):
    return [(TE.hexd(t), e1, e2) for t, e1, e2 in th.tm(pairs)]


def _check(name, pairs, got, want):
    bad = TE.mismatches(got, want)
    assert not bad, (name, len(bad), [(pairs[i], got[i], want[i]) for i in bad[:3]])


@pytest.fixture(scope="module")
def group_results():
    """dg_thal_batch on every corpus group, a batch each, at the default environment"""
    th = _thal("default")
    out = {name: _tm(th, pairs) for name, pairs in TC.groups().items()}
    th.close()
    return out


@pytest.mark.parametrize("name", list(TC.groups()))
def test_group_batch_equals_reference(group_results, name):
    pairs = TC.groups()[name]
    assert len(group_results[name]) == len(pairs) == len(TE.expected(name))
    _check(name, pairs, group_results[name], TE.expected(name))


def test_shared_pairs_do_not_depend_on_the_batch_they_travel_in(group_results):
    s8, s20 = TC.shared_pairs()
    seen = {}
    for L1, L2 in TC.GEOMETRIES:
        name = "geometry_%dx%d" % (L1, L2)
        at = {p: i for i, p in enumerate(TC.groups()[name])}
        for p in s8 + (s20 if L1 >= 20 and L2 >= 20 else []):
            got, want = group_results[name][at[p]], TE.expected(name)[at[p]]
            assert got == want[:3], (name, p, got, want)
            assert seen.setdefault(p, got) == got, (name, p)
    assert len(seen) == len(set(s8 + s20))


def test_one_shuffled_batch_of_everything_equals_the_group_batches(group_results):
    """wave pairs, long pairs and hand-backs interleaved: the redo bookkeeping of dg_thal_batch"""
    items = [(name, i) for name, pairs in TC.groups().items() for i in range(len(pairs))]
    random.Random(4).shuffle(items)
    pairs = [TC.groups()[n][i] for n, i in items]
    th = _thal("default")
    got = _tm(th, pairs)
    th.close()
    assert len(got) == sum(len(v) for v in TC.groups().values())
    bad = [(n, i) for (n, i), g in zip(items, got)
           if g[0] != group_results[n][i][0] or (TE.expected(n)[i][3] and g != group_results[n][i])]
    assert not bad, (len(bad), bad[:3])
    _check("all", pairs, got, [TE.expected(n)[i] for n, i in items])


@pytest.mark.parametrize("env", list(TC.ENVS))
def test_environment_batch_equals_reference(env):
    th = _thal(env)
    pairs = TC.env_pairs()
    got = _tm(th, pairs)
    th.close()
    assert len(got) == TC.N_ENV
    _check(env, pairs, got, TE.expected("env", env))


# ---- padlock: k_thal_self_wave ----------------------------------------------------------------------------------------------

_PCOMP = str.maketrans("ACGTUN", "TGCAAN")   # util.h:64 reverseComplement: U complements to A
NOT_COMPUTED = -1e300                        # DG_PADLOCK_NOT_COMPUTED


def _padlock_exons(armlen, seed):
    rng = random.Random(seed)
    T = 2 * armlen
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ex = [rnd(rng.randint(T + 20, 420)) for _ in range(14 if armlen >= 20 else 44)]   # (few short arms pass the Tm ceiling)
    ex.append(rnd(60) + "ACGT" * (T // 2) + rnd(40) + "GC" * armlen + "AT" * armlen + rnd(30))   # palindromic windows: the symmetric RC
    ex.append(rnd(T + 15) + "N" * 7 + rnd(T + 30) + "N" + rnd(T + 5))
    u = rnd(3 * T)
    ex.append(u[:T + 3] + "U" + u[T + 4:])
    ex.append(rnd(T))           # exactly one probe
    ex.append(rnd(T - 1))       # no position at all
    ex.append("AT" * (T + 10))  # low Tm, GC 0
    ex.append("".join(rng.choice("GC") for _ in range(T + 40)))   # GC 1, arms above the Tm ceiling at the longer arm lengths
    return ex


def _ref_self(windows):
    """{window: temperature} from the reference: thal(window, reverse complement)"""
    ws = sorted(set(windows))
    vals = TE.ref_values([(w, w.translate(_PCOMP)[::-1]) for w in ws], TC.ENVS["default"])
    assert all(v[3] for v in vals if len(ws[0]) <= 60)
    return {w: struct.unpack(">d", bytes.fromhex(v[0]))[0] for w, v in zip(ws, vals)}


@pytest.fixture(scope="module")
def tiny_index(tmp_path_factory):
    import dicey_amd
    seqs = make_genome(5, 2, 20000)
    fm9 = str(tmp_path_factory.mktemp("thalref") / "tiny.fm9")
    dicey_amd.build_index(genome_text(seqs), fm9)
    return fm9


@pytest.mark.parametrize("armlen", [8, 20, 24, 25, 30])
def test_padlock_scan_arm_and_probe_tm_equal_reference(tiny_index, armlen):
    """probe windows of 16, 40 and 48 nt are paired on the device (k_thal_self_wave, both instantiations), 50 and 60 go through
    dg_thal_batch.  The filter that decides which values exist (padlock.hip: arm_ok / probe_goes) is recomputed from the
    reference's values."""
    import dicey_amd
    L, T, tmdiff = armlen, 2 * armlen, 1000
    exons = _padlock_exons(armlen, 100 + armlen)
    with dicey_amd.FmIndex(tiny_index) as ix:
        th = _thal("default")
        R = dicey_amd.padlock_scan(ix, th, [e.encode() for e in exons], armlen=armlen, distance=0, tmdiff=tmdiff, gc_min=0.0, gc_max=1.0)
        arm_tm, probe_tm, arm_gc, probe_gc, off = (R[k].copy() for k in ("arm_tm", "probe_tm", "arm_gc", "probe_gc", "pos_off"))
        th.close()
    gc = lambda w: -1.0 if "N" in w else (w.count("C") + w.count("G")) / len(w)
    arm_ref = _ref_self([e[q:q + L] for e in exons for q in range(len(e) - L + 1) if len(e) >= T and "N" not in e[q:q + L]])
    n_arm = n_probe = n_arm_skipped = n_probe_skipped = 0
    want_probe = []
    for e, ex in enumerate(exons):
        npos = len(ex) - L + 1 if len(ex) >= T else 0
        assert int(off[e + 1] - off[e]) == npos
        for q in range(npos):
            at, w = int(off[e]) + q, ex[q:q + L]
            assert arm_gc[at] == gc(w)
            if "N" in w:
                assert arm_tm[at] == NOT_COMPUTED
                n_arm_skipped += 1
            else:
                assert TE.hexd(arm_tm[at]) == TE.hexd(arm_ref[w]), (armlen, w, arm_tm[at], arm_ref[w])
                n_arm += 1
        arm_ok = lambda q: "N" not in ex[q:q + L] and not (arm_ref[ex[q:q + L]] > 93 + gc(ex[q:q + L]) - 675.0 / armlen)
        for q in range(npos):
            at = int(off[e]) + q
            goes = q + T <= len(ex) and arm_ok(q) and arm_ok(q + L) and "N" not in ex[q:q + T] and \
                not abs(arm_ref[ex[q:q + L]] - arm_ref[ex[q + L:q + T]]) > tmdiff
            if q + T <= len(ex):
                assert probe_gc[at] == gc(ex[q:q + T])
            if goes:
                want_probe.append((at, ex[q:q + T]))
            else:
                assert probe_tm[at] == NOT_COMPUTED, (armlen, e, q)
                n_probe_skipped += 1
    probe_ref = _ref_self([w for _, w in want_probe])
    for at, w in want_probe:
        assert TE.hexd(probe_tm[at]) == TE.hexd(probe_ref[w]), (armlen, w, probe_tm[at], probe_ref[w])
        n_probe += 1
    assert R["n_arm_thal"] == n_arm and R["n_probe_thal"] == n_probe
    assert n_arm >= 3000 and n_probe >= 1000 and n_arm_skipped > 0 and n_probe_skipped > 0, (n_arm, n_probe, n_arm_skipped, n_probe_skipped)
    sym = [w for _, w in want_probe if w == revcomp(w)] + [w for w in arm_ref if L % 2 == 0 and w == revcomp(w)]
    assert sym and any("U" in w for w in arm_ref)


# ---- search: k_site_wave, k_site --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def search_genome(tmp_path_factory):
    import dicey_amd
    seqs = make_genome(77, 4, 400000)
    text = genome_text(seqs)
    fm9 = str(tmp_path_factory.mktemp("thalref_search") / "g.fm9")
    dicey_amd.build_index(text, fm9)
    return {"seqs": seqs, "text": text.decode(), "fm9": fm9, "seqlen": [len(s) + 1 for s in seqs]}


def _sample_primers(rng, seqs, n, lo, hi):
    out = []
    while len(out) < n:
        c, L = rng.randrange(len(seqs)), rng.randint(lo, hi)
        p = rng.randrange(0, len(seqs[c]) - L)
        s = seqs[c][p:p + L]
        if "N" in s:
            continue
        out.append(revcomp(s) if rng.random() < 0.5 else s)
    return out


def _edge_primers(rng, seqs, L=22):
    """primers whose k-mer matches within 30 nt of a chromosome's start or end while their 5' part hangs over the edge (the window
    is cut at the separator, silica.h:493-497), on either strand; and primers ending right next to an N run"""
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    out = []
    for s in seqs:
        for j in range(1, 7):
            for shift in (0, 3):
                head, tail = s[shift:shift + L - j], s[len(s) - shift - (L - j):len(s) - shift]
                if "N" not in head:
                    out += [rnd(j) + head, revcomp(head + rnd(j))]     # forward hit at the start; reverse-strand hit whose 3' k-mer sits there
                if "N" not in tail:
                    out += [revcomp(tail + rnd(j)), rnd(j) + tail]
        k, found = 0, 0
        while found < 6:
            k = s.find("N", k + 1)
            if k < 0:
                break
            if s[k - 1] != "N" and k > L and "N" not in s[k - L:k]:
                out += [s[k - L:k], revcomp(s[k - L:k])]
                found += 1
            e = k
            while e < len(s) and s[e] == "N":
                e += 1
            if e + L < len(s) and "N" not in s[e:e + L]:
                out += [s[e:e + L], revcomp(s[e:e + L])]
            k = e
    return out


def _within(q, c, d, hamming):
    if hamming or d == 0:
        return len(q) == len(c) and sum(x != y for x, y in zip(q, c)) <= d
    if abs(len(q) - len(c)) > d:
        return False
    prev = list(range(len(c) + 1))
    for i, x in enumerate(q, 1):
        cur = [i] + [0] * len(c)
        for j, y in enumerate(c, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[-1] <= d


def _candidate_windows(G, site, primer, kmer, distance, hamming):
    """The context windows thal() can have seen for this site (silica.h:474-500): every place near the site where a neighbour of
    the primer's k-mer occurs, with the 5' overhang and the context on both sides, cut at the separators and the text ends.
    The reported site is the window trimmed after the alignment (silica.h:538-549), so the window itself is recomputed here."""
    text, k = G["text"], kmer
    koff = len(primer) - k
    fwd = site["on_for"]
    q = primer[-k:] if fwd else revcomp(primer[-k:])
    ctx = 0 if hamming else distance
    pre0, post0 = (ctx + koff, ctx) if fwd else (ctx, ctx + koff)
    tpos = sum(G["seqlen"][:site["ref"]]) + site["pos"] - (1 << 32 if site["pos"] >= 1 << 31 else 0)
    span = koff + 3 * distance + 3
    h = k // 2
    wins = set()
    for loc in range(max(0, tpos - span), min(len(text), tpos + span + len(primer))):
        for mlen in ([k] if hamming else range(k - distance, k + distance + 1)):
            c = text[loc:loc + mlen]
            if len(c) < mlen or "\n" in c or (c[:h] != q[:h] and c[-h:] != q[-h:]) or not _within(q, c, distance, hamming):
                continue
            pre, post = min(pre0, loc), min(post0, len(text) - loc - mlen)
            left, right = text[loc - pre:loc], text[loc + mlen:loc + mlen + post]
            left = left[left.rfind("\n") + 1:]
            right = right.split("\n")[0]
            w = left + c + right
            if site["genome"] in w:
                wins.add(w)
    return wins


def _check_search(G, th, primers, **kw):
    import dicey_amd
    with dicey_amd.FmIndex(G["fm9"]) as ix:
        sites, match_temp, flags, nhits = dicey_amd.search_sites(ix, th, primers, G["seqlen"], cut_temp=-1.0e5, **kw)
    kmer, distance, hamming = kw.get("kmer", 15), kw.get("distance", 1), kw.get("hamming", False)
    perf = TE.ref_values([(p, revcomp(p)) for p in primers], TC.ENVS["default"])
    assert [TE.hexd(t) for t in match_temp] == [v[0] for v in perf]
    cands, jobs = [], []
    for s in sites:
        primer = primers[s["primer"]]
        assert TE.hexd(s["perf_temp"]) == perf[s["primer"]][0]
        pos = s["pos"] - (1 << 32 if s["pos"] >= 1 << 31 else 0)   # (alignpos - koffset is unsigned in the reference too)
        assert s["genome"] in G["seqs"][s["ref"]][max(0, pos - 80):pos + 160], s   # a piece of its chromosome: nothing from behind a separator
        o1 = revcomp(primer) if s["on_for"] else primer      # silica.h:502-509
        ws = sorted(_candidate_windows(G, s, primer, kmer, distance, hamming))
        assert ws, ("no hit of the k-mer explains this site", s, primer)
        cands.append(range(len(jobs), len(jobs) + len(ws)))
        jobs += [(o1, w) for w in ws]
    ref = TE.ref_values(jobs, TC.ENVS["default"])
    assert all(v[3] for v in ref)
    exact = 0
    for s, rng_ in zip(sites, cands):
        got = TE.hexd(s["temp"])
        assert got in {ref[i][0] for i in rng_}, (s, primers[s["primer"]], [(jobs[i], ref[i]) for i in rng_])
        if len(rng_) == 1 and jobs[rng_[0]][1] == s["genome"]:   # untrimmed: temp = thal(oligo1, site["genome"]) as it stands
            exact += 1
    assert min(struct.unpack(">d", bytes.fromhex(v[0]))[0] for v in ref) > -1.0e5   # the cut was below every temperature
    short = sum(1 for s in sites if len(s["genome"]) < len(primers[s["primer"]]))
    return len(sites), exact, short


SETTINGS = [dict(), dict(hamming=True, kmer=13), dict(distance=0)]   # as test_gpu_thal_wave.py, the cut below every temperature


@pytest.mark.parametrize("kw", SETTINGS, ids=["default", "hamming_k13", "distance0"])
def test_search_site_temperatures_equal_reference(search_genome, kw):
    G = search_genome
    rng = random.Random(21)
    th = _thal("default")
    try:
        # 16-27 nt plus the edge primers: the wave kernel (k_site_wave) and its window cuts
        n1, exact1, short1 = _check_search(G, th, _sample_primers(rng, G["seqs"], 300, 16, 27) + _edge_primers(rng, G["seqs"]), **kw)
        # 16-60 nt: windows too long for the wave kernel's LDS table, every hit goes to k_site (sequences packed in registers;
        # its byte-array variant needs a window above 82 nt, which no primer of at most 64 nt reaches)
        n2, exact2, short2 = _check_search(G, th, _sample_primers(rng, G["seqs"], 120, 16, 60) + _edge_primers(rng, G["seqs"], 40), **kw)
    finally:
        th.close()
    assert n1 >= 300 and n2 >= 120, (n1, n2)
    assert short1 >= 50 and short2 >= 20, (short1, short2)
    if kw.get("distance") == 0:
        assert exact1 + exact2 >= 300, (exact1, exact2)
