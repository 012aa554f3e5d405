#!/usr/bin/env python3
"""Time of one synchronous facet-count call on C2 (1M docs, BM25, ~0.55 M matches per query) beside the count call of
the same batch on the same snapshot: 256 queries, facets of 4 / 256 / 8192 values (doc % V).  Per V a warm-up of both
calls, then --reps alternating pairs: median and min - max of each and the ratio of the medians.
  --ab   instead: the replicated histogram against PS_FACET_REPLICAS=1 at V = 4 on a dense batch (every query the eight
         most frequent stems: nearly every document matches), a snapshot (engine) per leg, the legs alternating.
  --boosts 1,-0.5   the slow route (k_facet_runs behind stage 1 of the deep path)
The columns of EXPERIMENTS.md, each step under its own time limit and the chain ending at the first failure:
  timeout -k 10 400 python tools/facet_latency.py && timeout -k 10 400 python tools/facet_latency.py --ab
and the kernels' time per launch, in a run of its own:
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o kt -- python tools/facet_latency.py --reps 3"""
import argparse, hashlib, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--values", default="4,256,8192")
ap.add_argument("--boosts", default="1,1")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--ab", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import probly_search_amd as psa
from probly_search_amd import synth

cfg = dict(synth.CONFIGS["C2"])
c = synth.Corpus(**cfg)
index = synth.fill(psa.Index(cfg["fields"]), c)
sc, boosts = psa.bm25.new(), [float(b) for b in args.boosts.split(",")]
docs = np.arange(cfg["n_docs"], dtype=np.uint64)
print("library: %s  boosts: %s  batch: %d" % (psa.lib_path(), boosts, args.batch), flush=True)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def legs(named):
    """named: [(label, fn)] - a warm-up of each, then --reps rounds that run every leg once, in turn."""
    outs = [fn() for _, fn in named]
    ts = [[] for _ in named]
    for _ in range(args.reps):
        for i, (_, fn) in enumerate(named):
            ts[i].append(timed(fn)[0])
    for (label, _), t, o in zip(named, ts, outs):
        print("  %-28s median %.3f ms  min %.3f  max %.3f  (sum %d, sha256 %s)" % (
            label, float(np.median(t)), min(t), max(t), int(o.sum()), hashlib.sha256(np.asarray(o, np.uint64).tobytes()).hexdigest()[:16]), flush=True)
    return [float(np.median(t)) for t in ts]


if args.ab:
    qs = [" ".join(bytes(s).decode("ascii") for s in c.stems[:8])] * args.batch
    snaps = {}
    for r in ("0", "1"):
        os.environ["PS_FACET_REPLICAS"] = r  # read when the snapshot's engine is created
        snaps[r] = index.snapshot(device=0)
    facets = {r: s.facet(docs, (docs % 4).astype(np.uint32), 4) for r, s in snaps.items()}
    print("dense batch, V = 4:", flush=True)
    rep, one = legs([("replicated (rule)", lambda: snaps["0"].facet_counts_batch(qs, sc, boosts, facets["0"])),
                     ("PS_FACET_REPLICAS=1", lambda: snaps["1"].facet_counts_batch(qs, sc, boosts, facets["1"]))])
    print("  unreplicated / replicated = %.2f" % (one / rep), flush=True)
else:
    snap = index.snapshot(device=0)
    qs = c.queries(args.batch, cfg["q_terms"])
    for V in map(int, args.values.split(",")):
        facet = snap.facet(docs, (docs % V).astype(np.uint32), V)
        print("C2 B=%d V=%d:" % (args.batch, V), flush=True)
        cnt, fac = legs([("count_batch", lambda: snap.count_batch(qs, sc, boosts)),
                         ("facet_counts_batch", lambda: snap.facet_counts_batch(qs, sc, boosts, facet))])
        print("  facet / count = %.2f" % (fac / cnt), flush=True)
