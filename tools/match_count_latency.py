#!/usr/bin/env python3
"""Time of one synchronous total-match-count call on C2 (1M docs, BM25, ~0.55 M matches per query): batches of 24 / 256 /
1024 queries, a warm-up call, then median and min - max of --reps calls, plus a hash of the totals.
  --route count   Snapshot.count_batch (k_count_matches; with --boosts 1,0 its zero-boost instantiation, with
                  --boosts 1,-0.5 the slow route)
  --route top0    the only route a build without the count entry points has: query_batch(top_k=0) and len() per query
  --repo DIR      import the package (binding and library) of another checkout, e.g. the parent commit's
  --window N      PS_COUNT_WINDOW_LOG2 for this run (0: the engine's rule)
The columns of EXPERIMENTS.md, each step under its own time limit and the chain ending at the first failure:
  timeout -k 10 300 python tools/match_count_latency.py &&
  timeout -k 10 500 python tools/match_count_latency.py --route top0 --repo <parent checkout, built> --reps 5
and the kernel's time per launch, in a run of its own:
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o kt -- python tools/match_count_latency.py"""
import argparse, hashlib, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="24,256,1024")
ap.add_argument("--route", default="count", choices=["count", "top0"])
ap.add_argument("--boosts", default="1,1")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--window", type=int, default=0)
args = ap.parse_args()
if args.window:
    os.environ["PS_COUNT_WINDOW_LOG2"] = str(args.window)
sys.path.insert(0, os.path.abspath(args.repo))
import numpy as np
import probly_search_amd as psa
from probly_search_amd import synth

cfg = dict(synth.CONFIGS["C2"])
c = synth.Corpus(**cfg)
snap = synth.fill(psa.Index(cfg["fields"]), c).snapshot(device=0)
sc, boosts = psa.bm25.new(), [float(b) for b in args.boosts.split(",")]
print("library: %s  route: %s  boosts: %s  window: %s" % (psa.lib_path(), args.route, boosts, args.window or "rule"), flush=True)


def totals(qs):
    if args.route == "count":
        return snap.count_batch(qs, sc, boosts)
    return np.diff(snap.query_batch_arrays(qs, sc, None, boosts, 0)[2]).astype(np.uint64)


for B in map(int, args.batches.split(",")):
    qs = c.queries(B, cfg["q_terms"])
    tot = totals(qs)  # warm-up: buffers, code objects
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        totals(qs)
        ts.append((time.perf_counter() - t) * 1e3)
    print("C2 B=%-5d median %.3f ms  min %.3f  max %.3f  (postings %d, matches %d, sha256 %s)" % (
        B, float(np.median(ts)), min(ts), max(ts), snap.last_stats()["postings_visited"], int(tot.sum()),
        hashlib.sha256(np.asarray(tot, np.uint64).tobytes()).hexdigest()[:16]), flush=True)
