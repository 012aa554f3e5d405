#!/usr/bin/env python3
"""Conjunctive queries on C2 (1M docs, BM25, three-word queries): time of one synchronous query_batch_arrays call and of
the stage-1 kernel inside it (HIP events: ps_snapshot_kernel_breakdown, k_conj for match="all"), median of --reps calls
(200: a quarter of a second per leg) after three warm-up calls, the kernels' own work counts per query, and a hash of the answers.
  usage: tools/match_all_latency.py [--batch 256] [--ks 10,100] [--match all,any] [--reps 200] [--chunks 64,128,256]
--chunks: an A/B of PS_CONJ_CHUNK, the driver postings per work item - a snapshot (engine) per value over the same index.
A library from before match="all" takes --match any only (PS_SO=<its libprobly_search_amd.so>, with the binding of its
own checkout): the nearest route it has for the same batch is the deep top-k path at k = 100."""
import argparse, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import probly_search_amd as psa
from probly_search_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ks", default="10,100")
ap.add_argument("--match", default="all,any")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--chunks", default="")
args = ap.parse_args()
cfg = dict(synth.CONFIGS["C2"])
c = synth.Corpus(**cfg)
index = synth.fill(psa.Index(cfg["fields"]), c)
sc, boosts = psa.bm25.new(), [1.0] * cfg["fields"]
qs = c.queries(args.batch, cfg["q_terms"])
print("library: %s" % psa.lib_path(), flush=True)
runs = [(ch, m) for ch in args.chunks.split(",") for m in (["all"] if ch else args.match.split(","))]
for chunk, match in runs:
    if chunk:
        os.environ["PS_CONJ_CHUNK"] = chunk  # read when the snapshot's engine is created
        print("PS_CONJ_CHUNK=%s" % chunk, flush=True)
    snap = index.snapshot(device=0)
    kw = {"match": match} if match != "any" else {}
    for k in map(int, args.ks.split(",")):
        for _ in range(3):  # warm-up: buffers, code objects, the staging slots
            keys, scores, offs = snap.query_batch_arrays(qs, sc, None, boosts, k, **kw)
        h = hashlib.sha256(keys.tobytes() + scores.tobytes() + np.asarray(offs).tobytes()).hexdigest()[:16]
        snap.kernel_breakdown(reset=True)
        snap.work_counters(reset=True)
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            snap.query_batch_arrays(qs, sc, None, boosts, k, **kw)
            ts.append((time.perf_counter() - t) * 1e3)
        kb, wc = snap.kernel_breakdown(), snap.work_counters()
        per_q = 1.0 / (args.reps * args.batch)
        print("C2 B=%d match=%s k=%-4d call median %.3f ms  min %.3f  max %.3f | %s %.3f ms per call | per query: items %.1f "
              "postings scanned %.0f  reached %.1f  run elements %.1f | %d results, sha256 %s" % (
                  args.batch, match, k, float(np.median(ts)), min(ts), max(ts), kb["score_kernel"], kb["score_ms"] / max(1, kb["launches"]),
                  wc["items"] * per_q, (wc["postings_scanned"] + wc["k1_postings"]) * per_q, wc["postings_reached_lookups"] * per_q,
                  wc["run_results"] * per_q, len(keys), h), flush=True)
