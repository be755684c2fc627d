#!/usr/bin/env python3
"""Whole-genome timing of dg_mappability (include/dicey_gpu.h) and of `dicey mappability -o` — not the headline bench.  The genome
is bench.py's synthetic GRCh38-size text (--genome iid | repeats), generated on the device from a seed and indexed with
dg_index_build_device, or an existing index (--fm9).  Per k: device phase times from HIP events (dg_map_stats), both strands and
forward only; with --mismatches 1|2 the runs go through dg_mappability_mm ((k,e)-mappability) and report the search counters of
dg_map_mm_stats per head.  With --min-unique [--maxk K] the runs go through dg_min_unique instead (the shortest unique k-mer per
position): total, forward (neighbour prefixes) and reverse (the other strand's walk) ms, walk steps per position and, from the library's
DICEY_TIMING line, the longest launch of the walk — and beside each, on the same genome and build, ONE exact dg_mappability pass at
k = K: a bisection over 10..1000 needs seven of those.  With --min-unique --within e [--maxk K] the call is dg_min_unique_mm (the
shortest k-mer unique within e mismatches): total and search ms, candidates, probes / steps / table reads / verified rows per candidate
and the longest launch of the search -- and beside it ONE dg_mappability_mm(k = K, e) pass (the bisection the call replaces needs about
seven) and the exact dg_min_unique pass, on the same genome and build.  With --query the runs go through dg_query_map (k-mer counts for sequences
outside the index): one query set of 1 Mb cut from the genome with 1 % substitutions plus 1 Mb random, in records of 10 kb, at e = 0, 1, 2
per k, positions/s from the call's wall time and from the device time, the search counters per valid position, the longest launch — and,
at e = 0 in the same run, the route a build without dg_query_map offers to the same numbers: dg_count on every k-mer and its reverse
complement (cut out on the host, uploaded k-fold).  With --query --anchor A[,A..] the same query set goes through
dg_query_map_anchored (the last A bases of every k-mer matched exactly; `k` stands for the k-mer length) beside dg_query_map at the same k and e.
With --query --iupac [--degenerate-every N] the same query set goes through dg_query_map_iupac beside dg_query_map (on A/C/G/T records the
two queue the same search), and then, with a two-fold code that holds the base every N bases, beside the host's scan over expansions at
e = 0: with m = ceil(k / N) codes at most in a window, 2^m copies of the records (code j shows its member number bit (j mod m) of the copy's
index) go through dg_query_map and are summed, every window with c codes having met each of its expansions 2^(m-c) times.
With --query-minlen [--mismatches e] [--atmost t[,t..]] [--mink a --maxk b] [--no-scan] the same query
set goes through dg_query_min_len (the shortest specific k-mer per position), one warm-up call in front of the timed one: device and wall
ms, probes per valid position, the longest launch -- and beside it the route a build without it offers: one dg_query_map(k, max_count =
t + 1) per k in [a, b], combined on the host; `same_values` compares the two.  With --query-minlen --by-end [--anchor A[,A..]] the call is
dg_query_min_len_end (the shortest specific k-mer that ENDS at each position, its last A bases exact) and the scan beside it one
dg_query_map_anchored(k, A, max_count = t + 1) per k, each result shifted by k - 1 to the k-mer's last base on the host.  The CLI run reads names and lengths from a .fai written beside a stub FASTA (it never reads the sequence).
With --cover [--ks ..] each k gets one dg_mappability(k, max_count 2) call and the dg_map_cover transform of its map (at_most 1): the
transform's device ms (bitmap and directory, per-base kernel) beside the base call's ms_total of the same process; with --min-cover [--maxk K]
[--within e] the same for dg_min_unique / dg_min_unique_mm and dg_map_min_cover.
Prints one JSON line."""
import argparse, ctypes as C, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench, dicey_amd
from dicey_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--genome-size", type=float, default=3.1e9)
ap.add_argument("--genome", choices=["iid", "repeats"], default="iid")
ap.add_argument("--fm9", default="", help="reuse this index (its .lens.json beside it holds the sequence lengths)")
ap.add_argument("--ks", default="24,36,50,100,150")
ap.add_argument("--mismatches", type=int, default=0, help="e of (k,e)-mappability: 0 (exact), 1 or 2")
ap.add_argument("--min-unique", action="store_true", help="time dg_min_unique (max_k = --maxk) beside one exact pass at k = --maxk")
ap.add_argument("--maxk", type=int, default=100, help="max_k of --min-unique")
ap.add_argument("--within", type=int, default=0, help="with --min-unique: e of dg_min_unique_mm (1 or 2), timed beside one dg_mappability_mm(k = --maxk, e) "
                "pass and the exact dg_min_unique")
ap.add_argument("--cover", action="store_true", help="time dg_map_cover (per k of --ks, at_most 1) beside the dg_mappability call whose map it transforms")
ap.add_argument("--min-cover", action="store_true", help="time dg_map_min_cover (max_k = --maxk) beside the dg_min_unique call whose map it transforms")
ap.add_argument("--query", action="store_true", help="time dg_query_map on a 2 Mb query set (per k of --ks, e = 0, 1, 2) beside dg_count on its k-mers")
ap.add_argument("--query-mb", type=float, default=1.0, help="Mb of each half of the --query set (cut from the genome / random)")
ap.add_argument("--anchor", default="", help="with --query: time dg_query_map_anchored at these anchors (comma-separated; k = the k-mer length) beside "
                "dg_query_map at the same k and e (e = 1, 2, or --mismatches when given)")
ap.add_argument("--iupac", action="store_true", help="with --query: time dg_query_map_iupac beside dg_query_map on the A/C/G/T set, and on the set with a "
                "two-fold code every --degenerate-every bases beside a scan of dg_query_map over expansions at e = 0 (k at most 64)")
ap.add_argument("--degenerate-every", type=int, default=16, help="--iupac: bases between two codes of the degenerate set")
ap.add_argument("--query-minlen", action="store_true", help="time dg_query_min_len (--mink..--maxk, --mismatches, --atmost) beside a per-k scan of dg_query_map")
ap.add_argument("--by-end", action="store_true", help="--query-minlen: time dg_query_min_len_end (anchors of --anchor, default 0) beside a per-k scan "
                "of dg_query_map_anchored shifted to the k-mer's last base")
ap.add_argument("--mink", type=int, default=10, help="min_k of --query-minlen")
ap.add_argument("--atmost", default="0", help="at_most of --query-minlen; a comma-separated list gives one run each")
ap.add_argument("--no-scan", action="store_true", help="--query-minlen: skip the per-k scan of dg_query_map beside the call")
ap.add_argument("--maxcount", type=int, default=0, help="max_count of the runs (0 = exact values)")
ap.add_argument("--forward", choices=["both", "no", "yes"], default="both", help="which strand settings to time")
ap.add_argument("--keep-index", action="store_true", help="leave the generated index (and its .lens.json) in --workdir for --fm9 runs")
ap.add_argument("--cli-k", type=int, default=100, help="k of the end-to-end CLI run; 0 skips it")
ap.add_argument("--workdir", default="/dev/shm")
a = ap.parse_args()
if a.min_unique and (a.mismatches or a.maxcount):
    ap.error("--min-unique goes with neither --mismatches nor --maxcount")
if a.within and not (a.min_unique or a.min_cover):
    ap.error("--within goes with --min-unique or --min-cover")
if a.within not in (0, 1, 2):
    ap.error("--within is 0, 1 or 2")
if a.iupac and not a.query:
    ap.error("--iupac goes with --query")
if a.by_end and not a.query_minlen:
    ap.error("--by-end goes with --query-minlen")
dev = torch.device("cuda", 0)
L = _capi.load()
out = {"tool": "bench_mappability", "genome": a.genome, "genome_size": a.genome_size}
fm9 = a.fm9 or os.path.join(a.workdir, "dicey_map_bench_%s.fm9" % a.genome)
if not a.fm9:
    t0 = time.time()
    text, lens = bench.synth_genome(int(a.genome_size), 24, seed=1, device=dev, repeats=a.genome == "repeats")
    _capi.check(L, L.dg_index_build_device(C.c_void_p(text.data_ptr()), text.numel(), 0, fm9.encode()))
    json.dump([int(x) for x in lens], open(fm9 + ".lens.json", "w"))
    out["build_s"] = round(time.time() - t0, 2)
    del text
    torch.cuda.empty_cache()
lens = json.load(open(fm9 + ".lens.json"))
t0 = time.time()
ix = dicey_amd.FmIndex(fm9, compact=True, pre5=False)
out["open_s"] = round(time.time() - t0, 2)
n = ix.size()
out["n"] = n
runs = []
LINES_PER_S = 28e9  # what the search kernel sustains in random 64-byte lines: the yardstick of `line_share`

STRANDS = {"both": (False, True), "no": (False,), "yes": (True,)}[a.forward]


def stderr_of(call):
    """run call() with fd 2 in a file: what the library wrote to stderr meanwhile"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace")


def min_unique_run(fo):
    """one dg_min_unique pass at max_k = --maxk and, beside it, one exact dg_mappability pass at k = --maxk"""
    m, x = C.c_void_p(), C.c_void_p()
    prm = _capi.MinUniqueParams(a.maxk, 1 if fo else 0, 0, 0)
    os.environ["DICEY_TIMING"] = "1"
    t0 = time.time()
    err = stderr_of(lambda: _capi.check(L, L.dg_min_unique(ix.handle, C.byref(prm), C.byref(m))))
    wall = time.time() - t0
    del os.environ["DICEY_TIMING"]
    st = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(m, C.byref(st)))
    L.dg_map_free(m)
    line = re.search(r"min unique max_k=\d+: (\d+) launches of the walk, [0-9.]+ ms in all, longest ([0-9.]+) ms", err)
    xp = _capi.MapParams(a.maxk, 1 if fo else 0, 0, 0)
    _capi.check(L, L.dg_mappability(ix.handle, C.byref(xp), C.byref(x)))
    xs = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(x, C.byref(xs)))
    L.dg_map_free(x)
    return {"min_unique": True, "max_k": a.maxk, "forward_only": fo, "ms_total": round(st.ms_total, 1), "ms_forward": round(st.ms_forward, 1),
            "ms_reverse": round(st.ms_reverse, 1), "rev_steps": st.rev_steps, "steps_per_position": round(st.rev_steps / max(n - 1, 1), 3),
            "launches": int(line.group(1)) if line else None, "longest_launch_ms": float(line.group(2)) if line else None,
            "wall_s": round(wall, 2), "transient_gb": round(st.transient_bytes / 1e9, 2),
            "exact_pass_k": a.maxk, "exact_pass_ms_total": round(xs.ms_total, 1), "exact_pass_rev_steps": xs.rev_steps,
            "exact_pass_transient_gb": round(xs.transient_bytes / 1e9, 2),
            "cost_in_exact_passes": round(st.ms_total / max(xs.ms_total, 1e-9), 2)}


def cover_run(k, fo):
    """one dg_mappability pass at k (max_count 2: unique or not) and the cover transform of its map, at_most 1"""
    m, c = C.c_void_p(), C.c_void_p()
    prm = _capi.MapParams(k, 1 if fo else 0, 2, 0)
    _capi.check(L, L.dg_mappability(ix.handle, C.byref(prm), C.byref(m)))
    st = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(m, C.byref(st)))
    cp = _capi.CoverParams(1, a.maxcount, 0, 0)
    t0 = time.time()
    _capi.check(L, L.dg_map_cover(ix.handle, m, C.byref(cp), C.byref(c)))
    wall = time.time() - t0
    L.dg_map_free(m)
    cs = _capi.CoverStats()
    _capi.check(L, L.dg_map_cover_stats(c, C.byref(cs)))
    L.dg_map_free(c)
    ms = cs.ms_bits + cs.ms_cover
    return {"cover": True, "k": k, "forward_only": fo, "max_count": a.maxcount, "ms_transform": round(ms, 3), "ms_bits": round(cs.ms_bits, 3),
            "ms_cover": round(cs.ms_cover, 3), "wall_ms": round(wall * 1e3, 2), "specific": cs.specific, "covered": cs.covered,
            "transient_gb": round(cs.transient_bytes / 1e9, 3), "gb_per_s": round(8.4 * n / max(ms, 1e-9) / 1e6, 1),
            "base_ms_total": round(st.ms_total, 1), "transform_over_base": round(ms / max(st.ms_total, 1e-9), 4)}


def min_cover_run(fo):
    """one dg_min_unique pass at max_k = --maxk (--within e: dg_min_unique_mm) and the min-cover transform of its map"""
    m, c = C.c_void_p(), C.c_void_p()
    if a.within:
        prm = _capi.MinUniqueMmParams(a.maxk, a.within, 1 if fo else 0, 0, 0)
        _capi.check(L, L.dg_min_unique_mm(ix.handle, C.byref(prm), C.byref(m)))
    else:
        prm = _capi.MinUniqueParams(a.maxk, 1 if fo else 0, 0, 0)
        _capi.check(L, L.dg_min_unique(ix.handle, C.byref(prm), C.byref(m)))
    st = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(m, C.byref(st)))
    cp = _capi.MinCoverParams(0, 0)
    t0 = time.time()
    _capi.check(L, L.dg_map_min_cover(ix.handle, m, C.byref(cp), C.byref(c)))
    wall = time.time() - t0
    L.dg_map_free(m)
    cs = _capi.CoverStats()
    _capi.check(L, L.dg_map_cover_stats(c, C.byref(cs)))
    L.dg_map_free(c)
    return {"min_cover": True, "max_k": a.maxk, "within": a.within, "forward_only": fo, "ms_transform": round(cs.ms_cover, 3), "wall_ms": round(wall * 1e3, 2),
            "with_length": cs.specific, "covered": cs.covered, "gb_per_s": round(9.0 * n / max(cs.ms_cover, 1e-9) / 1e6, 1),
            "base_ms_total": round(st.ms_total, 1), "transform_over_base": round(cs.ms_cover / max(st.ms_total, 1e-9), 4)}


def min_unique_mm_run(fo):
    """one dg_min_unique_mm pass at max_k = --maxk, e = --within and, beside it, one dg_mappability_mm pass at k = --maxk with the same e and
    the exact dg_min_unique pass"""
    m, x, u = C.c_void_p(), C.c_void_p(), C.c_void_p()
    prm = _capi.MinUniqueMmParams(a.maxk, a.within, 1 if fo else 0, 0, 0)
    os.environ["DICEY_TIMING"] = "1"
    t0 = time.time()
    err = stderr_of(lambda: _capi.check(L, L.dg_min_unique_mm(ix.handle, C.byref(prm), C.byref(m))))
    wall = time.time() - t0
    del os.environ["DICEY_TIMING"]
    st, mu = _capi.MapStats(), _capi.MuMmStats()
    _capi.check(L, L.dg_map_stats(m, C.byref(st)))
    _capi.check(L, L.dg_map_mu_mm_stats(m, C.byref(mu)))
    L.dg_map_free(m)
    line = re.search(r"min unique max_k=\d+ e=\d+: (\d+) launches of the search, [0-9.]+ ms in all, longest ([0-9.]+) ms", err)
    xp = _capi.MapMmParams(a.maxk, a.within, 1 if fo else 0, 0, 0, 0)
    _capi.check(L, L.dg_mappability_mm(ix.handle, C.byref(xp), C.byref(x)))
    xs = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(x, C.byref(xs)))
    L.dg_map_free(x)
    up = _capi.MinUniqueParams(a.maxk, 1 if fo else 0, 0, 0)
    _capi.check(L, L.dg_min_unique(ix.handle, C.byref(up), C.byref(u)))
    us = _capi.MapStats()
    _capi.check(L, L.dg_map_stats(u, C.byref(us)))
    L.dg_map_free(u)
    c = max(mu.candidates, 1)
    return {"min_unique": True, "within": a.within, "max_k": a.maxk, "forward_only": fo, "ms_total": round(st.ms_total, 1),
            "ms_forward": round(st.ms_forward, 1), "ms_reverse": round(st.ms_reverse, 1), "ms_search": round(mu.ms_search, 1),
            "candidates": mu.candidates, "candidate_share": round(mu.candidates / max(n - 1, 1), 3), "probes_per_candidate": round(mu.probes / c, 2),
            "steps_per_candidate": round(mu.steps / c, 2), "table_reads_per_candidate": round(mu.table_reads / c, 2),
            "verified_rows_per_candidate": round(mu.verified_rows / c, 2), "launches": mu.launches,
            "longest_launch_ms": float(line.group(2)) if line else None, "wall_s": round(wall, 2), "transient_gb": round(st.transient_bytes / 1e9, 2),
            "mm_pass_k": a.maxk, "mm_pass_ms_total": round(xs.ms_total, 1), "mm_pass_transient_gb": round(xs.transient_bytes / 1e9, 2),
            "exact_min_unique_ms_total": round(us.ms_total, 1),
            "cost_in_mm_passes": round(st.ms_total / max(xs.ms_total, 1e-9), 2),
            "cost_over_seven_passes": round(st.ms_total / max(7 * xs.ms_total, 1e-9), 3)}


def query_set():
    """records of 10 kb: --query-mb Mb cut from the genome (pieces of 100 kb from seeded places) with 1 % substitutions, then as much random"""
    import numpy as np
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    half = int(a.query_mb * 1e6)
    piece = min(10_000, half)
    starts = [int(x) for x in rng.integers(0, n - 1 - piece, half // piece)]
    cut = np.frombuffer(b"".join(ix.extract([(p, p + piece - 1) for p in starts])), dtype=np.uint8).copy()
    hits = rng.integers(0, len(cut), len(cut) // 100)
    ok = np.isin(cut[hits], acgt)  # an N or a sequence end inside a piece stays what it is
    cut[hits[ok]] = acgt[rng.integers(0, 4, int(ok.sum()))]
    both = np.concatenate([cut, acgt[rng.integers(0, 4, half)]])
    return [both[i:i + 10_000].tobytes() for i in range(0, len(both), 10_000)]


def query_runs(k, recs):
    import numpy as np
    buf = b"".join(recs)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    vals = {}
    for e in (0, 1, 2):
        out_v = np.zeros(len(buf), dtype=np.uint32)
        prm = _capi.QmapParams(k, e, 0, a.maxcount, 0, (C.c_uint32 * 3)(0, 0, 0))
        st = _capi.QmapStats()
        _capi.check(L, L.dg_query_map(ix.handle, C.byref(prm), buf, off.ctypes.data_as(u64p), 1, out_v.ctypes.data_as(u32p), None))  # (warm-up: one record)
        os.environ["DICEY_TIMING"] = "1"
        t0 = time.time()
        err = stderr_of(lambda: _capi.check(L, L.dg_query_map(ix.handle, C.byref(prm), buf, off.ctypes.data_as(u64p), len(recs),
                                                                out_v.ctypes.data_as(u32p), C.byref(st))))
        wall = time.time() - t0
        del os.environ["DICEY_TIMING"]
        line = re.search(r"query map e=\d+: (\d+) launches of the search, [0-9.]+ ms in all, longest ([0-9.]+) ms", err)
        v = max(st.valid, 1)
        vals[e] = out_v
        runs.append({"query": True, "k": k, "mismatches": e, "max_count": a.maxcount, "positions": st.positions, "valid": st.valid,
                     "absent": int((out_v == 0).sum()), "wall_s": round(wall, 4), "ms_total": round(st.ms_total, 2), "ms_valid": round(st.ms_valid, 2),
                     "ms_search": round(st.ms_search, 2), "positions_per_s_wall": round(st.valid / wall), "positions_per_s_device": round(st.valid / max(st.ms_total, 1e-9) * 1e3),
                     "launches": st.launches, "longest_launch_ms": float(line.group(2)) if line else None, "early_exits": st.early_exits,
                     "steps_per_position": round(st.steps / v, 2), "table_reads_per_position": round(st.table_reads / v, 2),
                     "verified_rows_per_position": round(st.verified_rows / v, 2)})
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    # the other route to the e = 0 numbers: every valid k-mer and its reverse complement through dg_count
    t0 = time.time()
    b = np.frombuffer(buf, dtype=np.uint8)
    pos = np.nonzero(vals[0] != _capi.DG_QMAP_INVALID)[0]
    win = np.lib.stride_tricks.sliding_window_view(b, k)[pos]
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    pats = np.empty((len(pos), 2, k), dtype=np.uint8)
    pats[:, 0] = win
    pats[:, 1] = comp[win][:, ::-1]
    pbuf = pats.tobytes()
    poff = np.arange(0, 2 * len(pos) * k + 1, k, dtype=np.uint64)
    cut_s = time.time() - t0
    cnt = np.zeros(2 * len(pos), dtype=np.uint64)
    _capi.check(L, L.dg_count(ix.handle, pbuf, poff.ctypes.data_as(u64p), 1000, cnt.ctypes.data_as(u64p)))  # (warm-up: workspaces)
    t0 = time.time()
    _capi.check(L, L.dg_count(ix.handle, pbuf, poff.ctypes.data_as(u64p), 2 * len(pos), cnt.ctypes.data_as(u64p)))
    wall = time.time() - t0
    same = bool((cnt.reshape(-1, 2).sum(axis=1) == vals[0][pos]).all()) if a.maxcount == 0 else None
    runs.append({"query": True, "route": "dg_count per k-mer", "k": k, "mismatches": 0, "patterns": 2 * len(pos), "upload_mb": round(len(pbuf) / 1e6, 1),
                 "host_cut_s": round(cut_s, 3), "wall_s": round(wall, 4), "positions_per_s_wall": round(len(pos) / wall), "same_values": same})
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)


def query_anchor_runs(k, recs):
    """dg_query_map, then dg_query_map_anchored per anchor of --anchor, on the same records: one warm-up call in front of every timed one"""
    import numpy as np
    buf = b"".join(recs)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    offp = off.ctypes.data_as(u64p)
    anchors = [k if x == "k" else int(x) for x in a.anchor.split(",")]

    def timed(call, prm):
        vals = np.zeros(len(buf), dtype=np.uint32)
        st = _capi.QmapStats()
        _capi.check(L, call(ix.handle, C.byref(prm), buf, offp, len(recs), vals.ctypes.data_as(u32p), None))  # (warm-up)
        t0 = time.time()
        _capi.check(L, call(ix.handle, C.byref(prm), buf, offp, len(recs), vals.ctypes.data_as(u32p), C.byref(st)))
        return vals, st, time.time() - t0

    def row(st, wall):
        v = max(st.valid, 1)
        return {"valid": st.valid, "wall_ms": round(wall * 1e3, 2), "ms_total": round(st.ms_total, 2), "ms_search": round(st.ms_search, 2),
                "launches": st.launches, "steps_per_position": round(st.steps / v, 2), "table_reads_per_position": round(st.table_reads / v, 2),
                "verified_rows_per_position": round(st.verified_rows / v, 2)}

    for e in ([a.mismatches] if a.mismatches else [1, 2]):
        plain, st0, wall = timed(L.dg_query_map, _capi.QmapParams(k, e, 0, a.maxcount, 0, (C.c_uint32 * 3)(0, 0, 0)))
        exact = timed(L.dg_query_map, _capi.QmapParams(k, 0, 0, a.maxcount, 0, (C.c_uint32 * 3)(0, 0, 0)))[0]
        runs.append(dict({"query": True, "call": "dg_query_map", "k": k, "mismatches": e, "max_count": a.maxcount}, **row(st0, wall)))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        prev = plain
        for anc in anchors:
            vals, st, wall = timed(L.dg_query_map_anchored, _capi.QmapAnchorParams(k, e, anc, 0, a.maxcount, 0, (C.c_uint32 * 2)(0, 0)))
            ok = vals != _capi.DG_QMAP_INVALID
            runs.append(dict({"query": True, "call": "dg_query_map_anchored", "k": k, "mismatches": e, "anchor": anc, "max_count": a.maxcount,
                              "over_dg_query_map": round(st.ms_search / max(st0.ms_search, 1e-9), 3), "below_unanchored": int((vals[ok] < plain[ok]).sum()),
                              "above_exact": int((vals[ok] > exact[ok]).sum()), "never_above_smaller_anchor": bool((vals <= prev).all())}, **row(st, wall)))
            if anc == 0:
                runs[-1]["same_values"] = bool((vals == plain).all())
            if anc == k:
                runs[-1]["same_values"] = bool((vals == exact).all())
            prev = vals
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)


def query_iupac_runs(k, recs):
    """dg_query_map and dg_query_map_iupac on the A/C/G/T records, then dg_query_map_iupac on the degenerate set beside the scan over
    expansions: one warm-up call in front of every timed one"""
    import numpy as np
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    offp = off.ctypes.data_as(u64p)
    INV = _capi.DG_QMAP_INVALID

    def timed(call, prm, st, buf):
        vals = np.zeros(len(buf), dtype=np.uint32)
        _capi.check(L, call(ix.handle, C.byref(prm), buf, offp, len(recs), vals.ctypes.data_as(u32p), None))  # (warm-up)
        t0 = time.time()
        _capi.check(L, call(ix.handle, C.byref(prm), buf, offp, len(recs), vals.ctypes.data_as(u32p), C.byref(st)))
        return vals, st, time.time() - t0

    def row(st, wall):
        v = max(st.valid, 1)
        return {"valid": st.valid, "wall_ms": round(wall * 1e3, 2), "ms_total": round(st.ms_total, 2), "ms_search": round(st.ms_search, 2),
                "launches": st.launches, "steps_per_position": round(st.steps / v, 2), "table_reads_per_position": round(st.table_reads / v, 2),
                "verified_rows_per_position": round(st.verified_rows / v, 2)}

    plain_p = lambda e: _capi.QmapParams(k, e, 0, a.maxcount, 0, (C.c_uint32 * 3)(0, 0, 0))
    # max_degeneracy 1 on the A/C/G/T set: a k-mer with an N of the genome is invalid there as it is for dg_query_map; the default (256) on
    # the degenerate set.  A lane walks the expansions of its k-mer one after the other, so the largest degeneracy sets the call's tail
    iupac_p = lambda e, maxdeg: _capi.QmapIupacParams(k, e, 0, 0, a.maxcount, maxdeg, 0, (C.c_uint32 * 3)(0, 0, 0))
    buf = b"".join(recs)
    # the degenerate set: every N-th base, record by record, becomes the two-fold code of itself and `alt`
    every, m = a.degenerate_every, -(-k // a.degenerate_every)
    code, alt = np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8)
    code[list(b"ACGT")], alt[list(b"ACGT")] = list(b"RYKW"), list(b"GTTA")
    base = np.frombuffer(buf, dtype=np.uint8)
    at = np.concatenate([int(off[i]) + np.arange(every // 2, len(r), every) for i, r in enumerate(recs)])
    at = at[np.isin(base[at], np.frombuffer(b"ACGT", dtype=np.uint8))]
    deg = base.copy()
    deg[at] = code[base[at]]
    in_rec = at - off[np.searchsorted(off, at, side="right") - 1].astype(np.int64)
    number = (in_rec - every // 2) // every  # consecutive codes of a record have consecutive numbers: distinct mod m inside a window
    ncodes = np.zeros(len(base) + 1, dtype=np.int64)
    ncodes[1:] = np.cumsum(deg != base)
    for e in ([a.mismatches] if a.mismatches else [0, 1, 2]):
        plain, st0, wall0 = timed(L.dg_query_map, plain_p(e), _capi.QmapStats(), buf)
        runs.append(dict({"query": True, "call": "dg_query_map", "set": "acgt", "k": k, "mismatches": e, "max_count": a.maxcount}, **row(st0, wall0)))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        vals, st, wall = timed(L.dg_query_map_iupac, iupac_p(e, 1), _capi.QmapIupacStats(), buf)
        ok = plain != INV
        runs.append(dict({"query": True, "call": "dg_query_map_iupac", "set": "acgt", "k": k, "mismatches": e, "max_count": a.maxcount,
                          "over_dg_query_map": round(st.ms_search / max(st0.ms_search, 1e-9), 3), "same_values": bool((vals == plain).all()),
                          "same_counters": [st.valid, st.steps, st.table_reads, st.verified_rows] == [st0.valid, st0.steps, st0.table_reads, st0.verified_rows]},
                         **row(st, wall)))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        dvals, dst, dwall = timed(L.dg_query_map_iupac, iupac_p(e, 0), _capi.QmapIupacStats(), deg.tobytes())
        runs.append(dict({"query": True, "call": "dg_query_map_iupac", "set": "degenerate", "degenerate_every": every, "k": k, "mismatches": e,
                          "max_count": a.maxcount, "degenerate": dst.degenerate, "too_degenerate": dst.too_degenerate,
                          "expansions_per_position": round(dst.expansions / max(dst.valid, 1), 2)}, **row(dst, dwall)))
        if e == 0 and a.maxcount == 0:
            t0 = time.time()
            total, ms = np.zeros(len(base), dtype=np.int64), 0.0
            for c in range(1 << m):
                copy = base.copy()
                take = ((c >> (number % m)) & 1).astype(bool)
                copy[at[take]] = alt[base[at[take]]]
                v, sc, _ = timed(L.dg_query_map, plain_p(0), _capi.QmapStats(), copy.tobytes())
                total += np.where(v == INV, 0, v)
                ms += sc.ms_total
            win = ncodes[np.minimum(np.arange(len(base)) + k, len(base))] - ncodes[:-1]
            total >>= np.maximum(m - win, 0)  # a window with c codes met each of its expansions 2^(m-c) times
            runs[-1].update({"scan_calls": 1 << m, "scan_ms_total": round(ms, 2), "scan_wall_ms": round((time.time() - t0) * 1e3, 2),
                             "scan_over_call": round(ms / max(dst.ms_total, 1e-9), 2), "same_values": bool((total[ok] == dvals[ok]).all())})
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)


def query_minlen_run(recs, t):
    import numpy as np
    buf = b"".join(recs)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    offp = off.ctypes.data_as(u64p)
    INV = _capi.DG_QMAP_INVALID
    e = a.mismatches
    got = np.zeros(len(buf), dtype=np.uint32)
    prm = _capi.QminlenParams(a.mink, a.maxk, e, 0, t, 0, (C.c_uint32 * 2)(0, 0))
    st = _capi.QminlenStats()
    _capi.check(L, L.dg_query_min_len(ix.handle, C.byref(prm), buf, offp, len(recs), got.ctypes.data_as(u32p), None))  # (warm-up)
    os.environ["DICEY_TIMING"] = "1"
    t0 = time.time()
    err = stderr_of(lambda: _capi.check(L, L.dg_query_min_len(ix.handle, C.byref(prm), buf, offp, len(recs), got.ctypes.data_as(u32p), C.byref(st))))
    wall = time.time() - t0
    del os.environ["DICEY_TIMING"]
    line = re.search(r"query min length e=\d+: (\d+) launches of the search, [0-9.]+ ms in all, longest ([0-9.]+) ms", err)
    v = max(st.valid, 1)
    run = {"query_minlen": True, "min_k": a.mink, "max_k": a.maxk, "mismatches": e, "at_most": t, "positions": st.positions, "valid": st.valid,
           "found": st.found, "wall_ms": round(wall * 1e3, 2), "ms_total": round(st.ms_total, 2), "ms_valid": round(st.ms_valid, 2),
           "ms_search": round(st.ms_search, 2), "launches": st.launches, "longest_launch_ms": float(line.group(2)) if line else None,
           "probes_per_position": round(st.probes / v, 2), "steps_per_position": round(st.steps / v, 2),
           "table_reads_per_position": round(st.table_reads / v, 2), "verified_rows_per_position": round(st.verified_rows / v, 2)}
    if a.no_scan:
        return run
    # the route without dg_query_min_len: one dg_query_map per k with max_count = t + 1, the first k with a value <= t taken on the host
    vals = np.zeros(len(buf), dtype=np.uint32)
    qp = _capi.QmapParams(a.mink, e, 0, t + 1, 0, (C.c_uint32 * 3)(0, 0, 0))
    _capi.check(L, L.dg_query_map(ix.handle, C.byref(qp), buf, offp, 1, vals.ctypes.data_as(u32p), None))  # (warm-up: one record)
    scan = None
    dev_ms = 0.0
    t0 = time.time()
    for k in range(a.mink, a.maxk + 1):
        qp = _capi.QmapParams(k, e, 0, t + 1, 0, (C.c_uint32 * 3)(0, 0, 0))
        qs = _capi.QmapStats()
        _capi.check(L, L.dg_query_map(ix.handle, C.byref(qp), buf, offp, len(recs), vals.ctypes.data_as(u32p), C.byref(qs)))
        dev_ms += qs.ms_total
        if scan is None:
            scan = np.where(vals == INV, INV, 0).astype(np.uint32)
        scan[(scan == 0) & (vals != INV) & (vals <= t)] = k
    scan_wall = time.time() - t0
    run.update({"scan_calls": a.maxk - a.mink + 1, "scan_wall_ms": round(scan_wall * 1e3, 2), "scan_ms_total": round(dev_ms, 2),
                "same_values": bool((scan == got).all()), "scan_over_call_wall": round(scan_wall / max(wall, 1e-9), 2),
                "scan_over_call_device": round(dev_ms / max(st.ms_total, 1e-9), 2)})
    return run


def query_minlen_end_run(recs, t, anc):
    import numpy as np
    buf = b"".join(recs)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    offp = off.ctypes.data_as(u64p)
    INV = _capi.DG_QMAP_INVALID
    e = a.mismatches
    got = np.zeros(len(buf), dtype=np.uint32)
    prm = _capi.QminlenEndParams(a.mink, a.maxk, e, anc, 0, t, 0, (C.c_uint32 * 2)(0, 0))
    st = _capi.QminlenStats()
    _capi.check(L, L.dg_query_min_len_end(ix.handle, C.byref(prm), buf, offp, len(recs), got.ctypes.data_as(u32p), None))  # (warm-up)
    os.environ["DICEY_TIMING"] = "1"
    t0 = time.time()
    err = stderr_of(lambda: _capi.check(L, L.dg_query_min_len_end(ix.handle, C.byref(prm), buf, offp, len(recs), got.ctypes.data_as(u32p), C.byref(st))))
    wall = time.time() - t0
    del os.environ["DICEY_TIMING"]
    line = re.search(r"query min length by end e=\d+ anchor=\d+: (\d+) launches of the search, [0-9.]+ ms in all, longest ([0-9.]+) ms", err)
    v = max(st.valid, 1)
    run = {"query_minlen_end": True, "min_k": a.mink, "max_k": a.maxk, "mismatches": e, "anchor": anc, "at_most": t, "positions": st.positions,
           "valid": st.valid, "found": st.found, "wall_ms": round(wall * 1e3, 2), "ms_total": round(st.ms_total, 2), "ms_valid": round(st.ms_valid, 2),
           "ms_search": round(st.ms_search, 2), "launches": st.launches, "longest_launch_ms": float(line.group(2)) if line else None,
           "probes_per_position": round(st.probes / v, 2), "steps_per_position": round(st.steps / v, 2),
           "table_reads_per_position": round(st.table_reads / v, 2), "verified_rows_per_position": round(st.verified_rows / v, 2)}
    if a.no_scan:
        return run
    # the route without dg_query_min_len_end: one dg_query_map_anchored per k with max_count = t + 1, every result shifted by k - 1 to the
    # k-mer's last base inside its record, the first k with a value <= t taken on the host
    vals = np.zeros(len(buf), dtype=np.uint32)
    rec_of = np.repeat(np.arange(len(recs)), [len(r) for r in recs])
    in_rec = np.arange(len(buf)) - off[:-1].astype(np.int64)[rec_of]
    qp = _capi.QmapAnchorParams(a.mink, e, anc, 0, t + 1, 0, (C.c_uint32 * 2)(0, 0))
    _capi.check(L, L.dg_query_map_anchored(ix.handle, C.byref(qp), buf, offp, 1, vals.ctypes.data_as(u32p), None))  # (warm-up: one record)
    scan = None
    dev_ms = 0.0
    t0 = time.time()
    for k in range(a.mink, a.maxk + 1):
        qp = _capi.QmapAnchorParams(k, e, anc, 0, t + 1, 0, (C.c_uint32 * 2)(0, 0))
        qs = _capi.QmapStats()
        _capi.check(L, L.dg_query_map_anchored(ix.handle, C.byref(qp), buf, offp, len(recs), vals.ctypes.data_as(u32p), C.byref(qs)))
        dev_ms += qs.ms_total
        end = np.full(len(buf), INV, dtype=np.uint32)
        end[k - 1:] = vals[:len(buf) - k + 1]
        end[in_rec < k - 1] = INV  # (a value shifted in from the record in front)
        if scan is None:
            scan = np.where(end == INV, INV, 0).astype(np.uint32)
        scan[(scan == 0) & (end != INV) & (end <= t)] = k
    scan_wall = time.time() - t0
    run.update({"scan_calls": a.maxk - a.mink + 1, "scan_wall_ms": round(scan_wall * 1e3, 2), "scan_ms_total": round(dev_ms, 2),
                "same_values": bool((scan == got).all()), "scan_over_call_wall": round(scan_wall / max(wall, 1e-9), 2),
                "scan_over_call_device": round(dev_ms / max(st.ms_total, 1e-9), 2)})
    return run


if a.query_minlen:
    recs = query_set()
    for t in [int(x) for x in a.atmost.split(",")]:
        if a.by_end:
            for anc in [int(x) for x in (a.anchor or "0").split(",")]:
                runs.append(query_minlen_end_run(recs, t, anc))
                print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
            continue
        runs.append(query_minlen_run(recs, t))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    ks = []
elif a.query:
    recs = query_set()
    for k in [int(x) for x in a.ks.split(",")]:
        if a.iupac:
            query_iupac_runs(k, recs)
        elif a.anchor:
            query_anchor_runs(k, recs)
        else:
            query_runs(k, recs)
    ks = []
elif a.cover or a.min_cover:
    for fo in STRANDS:
        for k in ([int(x) for x in a.ks.split(",")] if a.cover else [a.maxk]):
            runs.append(cover_run(k, fo) if a.cover else min_cover_run(fo))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    ks = []
elif a.min_unique:
    for fo in STRANDS:
        runs.append(min_unique_mm_run(fo) if a.within else min_unique_run(fo))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    ks = []
else:
    ks = [int(x) for x in a.ks.split(",")]
for k in ks:
    for fo in STRANDS:
        m = C.c_void_p()
        t0 = time.time()
        if a.mismatches:
            prm = _capi.MapMmParams(k, a.mismatches, 1 if fo else 0, a.maxcount, 0, 0)
            _capi.check(L, L.dg_mappability_mm(ix.handle, C.byref(prm), C.byref(m)))
        else:
            prm = _capi.MapParams(k, 1 if fo else 0, a.maxcount, 0)
            _capi.check(L, L.dg_mappability(ix.handle, C.byref(prm), C.byref(m)))
        wall = time.time() - t0
        st = _capi.MapStats()
        _capi.check(L, L.dg_map_stats(m, C.byref(st)))
        mm = _capi.MapMmStats()
        _capi.check(L, L.dg_map_mm_stats(m, C.byref(mm)))
        L.dg_map_free(m)
        runs.append({"k": k, "mismatches": a.mismatches, "max_count": a.maxcount, "forward_only": fo, "ms_total": round(st.ms_total, 1),
                     "ms_valid": round(st.ms_valid, 1),
                     "ms_forward": round(st.ms_forward, 1), "ms_reverse": round(st.ms_reverse, 1), "ms_scatter": round(st.ms_scatter, 1),
                     "forward_share": round((st.ms_valid + st.ms_forward + st.ms_scatter) / max(st.ms_total, 1e-9), 3),
                     "rev_steps": st.rev_steps, "wall_s": round(wall, 2), "transient_gb": round(st.transient_bytes / 1e9, 2)})
        if a.mismatches:
            h = max(mm.heads, 1)
            # random lines: two Occ lines per step, one table line per read, per verified row one suffix-array line and the text lines
            # of the remaining characters (at least one)
            lines = 2 * mm.steps + mm.table_reads + 2 * mm.verified_rows
            runs[-1].update({"heads": mm.heads, "launches": mm.launches, "early_exits": mm.early_exits, "ms_search": round(mm.ms_search, 1),
                             "steps_per_head": round(mm.steps / h, 2), "table_reads_per_head": round(mm.table_reads / h, 2),
                             "verified_rows_per_head": round(mm.verified_rows / h, 2), "lines_per_head": round(lines / h, 1),
                             "line_share": round(lines / max(mm.ms_search, 1e-9) * 1e3 / LINES_PER_S, 3)})
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
out["runs"] = runs
ix.close()
# the CLI end to end: open + map + runs + format + gzip
stem = os.path.join(a.workdir, "dicey_map_bench_cli_%s" % a.genome)
gz = stem + ".bedgraph.gz"
if a.cli_k and not a.min_unique and not a.cover and not a.min_cover and not a.query and not a.query_minlen:
    with open(stem + ".fa", "w") as f:
        f.write(">chr1\nN\n")
    with open(stem + ".fa.fai", "w") as f:
        for i, l in enumerate(lens):
            f.write("chr%d\t%d\t0\t60\t61\n" % (i + 1, l))
    if os.path.lexists(stem + ".fm9"):
        os.remove(stem + ".fm9")
    os.symlink(os.path.abspath(fm9), stem + ".fm9")
    t0 = time.time()
    r = subprocess.run([os.path.join(ROOT, "dicey_amd", "dicey"), "mappability", "-g", stem + ".fa", "-k", str(a.cli_k), "-e", str(a.mismatches), "-c", str(a.maxcount),
                        "-o", gz],
                       capture_output=True, text=True)
    out["cli"] = {"k": a.cli_k, "mismatches": a.mismatches, "max_count": a.maxcount, "rc": r.returncode, "wall_s": round(time.time() - t0, 2),
                  "gz_bytes": os.path.getsize(gz) if os.path.exists(gz) else 0, "stderr": r.stderr[-300:]}
for p in (gz, stem + ".fm9", stem + ".fa", stem + ".fa.fai") + (() if a.fm9 or a.keep_index else (fm9, fm9 + ".lens.json")):
    if os.path.lexists(p):
        os.remove(p)
print(json.dumps(out))
