#!/usr/bin/env python3
"""Looks for oligo pairs in which an opening candidate with S < -2500 wins during the table fill (thal.h:1322-1330) — the one
case the wave kernel (thal_wave.hpp) does not compute itself but hands to the sequential kernel.  Runs the host build of thal.hpp
with its counter (tests/host/thal_host.cpp) over the test corpus and N extra pairs of 30-48 nt with long AT-rich loops.
Usage: thal_cutoff_search.py [N=200000].  Prints the count and the first ten pairs; DESIGN.md (thal section) records the result."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import thal_corpus as TC   # noqa: E402
import thal_expect as TE   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
found, seen = [], 0
sets = [(name, pairs, "default") for name, pairs in TC.groups().items()] + [("env", TC.env_pairs(), e) for e in TC.ENVS]
extra = TC.cutoff_search_pairs(n)
sets += [("extra", extra[k:k + 20000], "default") for k in range(0, n, 20000)]
for name, pairs, env in sets:
    wins = []
    TE.host_values(pairs, TC.ENVS[env], wins)
    seen += len(pairs)
    found += [(name, env, p, w) for p, w in zip(pairs, wins) if w]
print("pairs examined: %d, pairs with a winning cut-off candidate: %d" % (seen, len(found)))
for f in found[:10]:
    print(f)
