#!/usr/bin/env python3
"""Whole-genome timing of dg_mappability (include/dicey_gpu.h) and of `dicey mappability -o` — not the headline bench.  The genome
is bench.py's synthetic GRCh38-size text (--genome iid | repeats), generated on the device from a seed and indexed with
dg_index_build_device, or an existing index (--fm9).  Per k: device phase times from HIP events (dg_map_stats), both strands and
forward only; with --mismatches 1|2 the runs go through dg_mappability_mm ((k,e)-mappability) and report the search counters of
dg_map_mm_stats per head.  With --min-unique [--maxk K] the runs go through dg_min_unique instead (the shortest unique k-mer per
position): total, forward (neighbour prefixes) and reverse (the other strand's walk) ms, walk steps per position and, from the library's
DICEY_TIMING line, the longest launch of the walk — and beside each, on the same genome and build, ONE exact dg_mappability pass at
k = K: a bisection over 10..1000 needs seven of those.  The CLI run reads names and lengths from a .fai written beside a stub FASTA (it never reads the sequence).
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
ap.add_argument("--maxcount", type=int, default=0, help="max_count of the runs (0 = exact values)")
ap.add_argument("--forward", choices=["both", "no", "yes"], default="both", help="which strand settings to time")
ap.add_argument("--keep-index", action="store_true", help="leave the generated index (and its .lens.json) in --workdir for --fm9 runs")
ap.add_argument("--cli-k", type=int, default=100, help="k of the end-to-end CLI run; 0 skips it")
ap.add_argument("--workdir", default="/dev/shm")
a = ap.parse_args()
if a.min_unique and (a.mismatches or a.maxcount):
    ap.error("--min-unique goes with neither --mismatches nor --maxcount")
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


if a.min_unique:
    for fo in STRANDS:
        runs.append(min_unique_run(fo))
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
if a.cli_k and not a.min_unique:
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
