#!/usr/bin/env python3
"""Time of one synchronous query_batch on C2 (1M docs, BM25) for top_k above the per-lane top-k limit: batches of 24 /
256 / 1024 queries at k = 100 and k = 1000, median of --reps calls after a warm-up call, plus a hash of the answers.
Run it once per library to compare two builds (PS_SO=<other libprobly_search_amd.so>): up to k = 1024 this head selects
on the device (k_deep_select), an older build serves the same call through full-result mode; the hashes must agree.
  usage: tools/deep_topk_latency.py [--batches 24,256,1024] [--ks 100,1000] [--reps 5] [--skip 0,1000,100000]
--skip: result pages - ranks [skip, skip + k) of every query, selected on the device by k_deep_window (skip = 0 is the
plain call; a library older than the paged entry points takes only that).
The two columns of EXPERIMENTS.md, every GPU step under a time limit of its own and the chain ending at the first failure
(<parent> = a checkout of the parent commit with its library built):
  timeout -k 10 400 python tools/deep_topk_latency.py &&
  PS_SO=<parent>/probly-search_amd/csrc/libprobly_search_amd.so timeout -k 10 400 python tools/deep_topk_latency.py
and k_deep_select's time per launch, in a run of its own:
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o kt -- python tools/deep_topk_latency.py --reps 3"""
import argparse, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import probly_search_amd as psa
from probly_search_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="24,256,1024")
ap.add_argument("--ks", default="100,1000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip", default="0")
args = ap.parse_args()
cfg = dict(synth.CONFIGS["C2"])
c = synth.Corpus(**cfg)
snap = synth.fill(psa.Index(cfg["fields"]), c).snapshot(device=0)
sc, boosts = psa.bm25.new(), [1.0] * cfg["fields"]
print("library: %s" % psa.lib_path(), flush=True)
for B in map(int, args.batches.split(",")):
    qs = c.queries(B, cfg["q_terms"])
    for k, skip in ((k, s) for k in map(int, args.ks.split(",")) for s in map(int, args.skip.split(","))):
        page = {"skip": skip} if skip else {}
        keys, scores, offs = snap.query_batch_arrays(qs, sc, None, boosts, k, **page)  # warm-up: buffers, code objects
        h = hashlib.sha256(keys.tobytes() + scores.tobytes() + np.asarray(offs).tobytes()).hexdigest()[:16]
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            snap.query_batch_arrays(qs, sc, None, boosts, k, **page)
            ts.append((time.perf_counter() - t) * 1e3)
        print("C2 B=%-5d k=%-5d%s median %.3f ms  min %.3f  max %.3f  (%d results, sha256 %s)" % (
            B, k, " skip=%-7d" % skip if skip else "", float(np.median(ts)), min(ts), max(ts), len(keys), h), flush=True)
