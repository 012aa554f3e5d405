#!/usr/bin/env python3
"""Document filters on C2 (1M docs, BM25, three-word queries): time of one synchronous filtered call and of the stage-1
kernel inside it (HIP events: ps_snapshot_kernel_breakdown), median of --reps calls after three warm-up calls, for filters
of --fractions of the documents (a seeded random sample of the keys), at every k of --ks and for count_batch, under
PS_FILTER_DRIVE=1 (k_filter_score: the filter drives) and =0 (the lists drive under the allow bitmap) - a snapshot
(engine) per value over the same index, the legs of one filter alternating between them - and the unfiltered call at the
same k, which a library from before filters can run too: the yardstick.
  usage: tools/filter_latency.py [--batch 256] [--ks 10,100] [--fractions 0.001,0.05,0.5] [--reps 200] [--match any]"""
import argparse, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import probly_search_amd as psa
from probly_search_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ks", default="10,100")
ap.add_argument("--fractions", default="0.001,0.05,0.5")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--match", default="any")
args = ap.parse_args()
cfg = dict(synth.CONFIGS["C2"])
c = synth.Corpus(**cfg)
index = synth.fill(psa.Index(cfg["fields"]), c)
sc, boosts = psa.bm25.new(), [1.0] * cfg["fields"]
qs = c.queries(args.batch, cfg["q_terms"])
print("library: %s" % psa.lib_path(), flush=True)
snaps = {}
for drive in ("1", "0"):
    os.environ["PS_FILTER_DRIVE"] = drive  # read when the snapshot's engine is created
    snaps[drive] = index.snapshot(device=0)


def leg(name, snap, call, count):
    for _ in range(3):  # warm-up: buffers, code objects, the staging slots
        out = call()
    h = hashlib.sha256(b"".join(np.asarray(x).tobytes() for x in (out if isinstance(out, tuple) else (out,)))).hexdigest()[:16]
    snap.kernel_breakdown(reset=True)
    snap.work_counters(reset=True)
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    kb, wc = snap.kernel_breakdown(), snap.work_counters()
    per_q = 1.0 / (args.reps * args.batch)
    stage1 = "(no stage-1 timer)" if count and not kb["launches"] else "%s %.3f ms per launch" % (kb["score_kernel"], kb["score_ms"] / max(1, kb["launches"]))
    print("%-34s call median %.3f ms  min %.3f  max %.3f | %s | per query: items %.1f  scanned %.0f  reached %.1f | sha256 %s" % (
        name, float(np.median(ts)), min(ts), max(ts), stage1, wc["items"] * per_q,
        (wc["postings_scanned"] + wc["k1_postings"]) * per_q, wc["postings_reached_lookups"] * per_q, h), flush=True)


kw = {"match": args.match} if args.match != "any" else {}
for k in map(int, args.ks.split(",")):
    leg("unfiltered k=%d" % k, snaps["0"], lambda: snaps["0"].query_batch_arrays(qs, sc, None, boosts, k, **kw), False)
leg("unfiltered count", snaps["0"], lambda: snaps["0"].count_batch(qs, sc, boosts, **kw), True)
rng = np.random.default_rng(7)
for frac in map(float, args.fractions.split(",")):
    keys = rng.choice(cfg["n_docs"], size=max(1, int(cfg["n_docs"] * frac)), replace=False).astype(np.uint64)
    t = time.perf_counter()
    fs = {d: s.filter(keys) for d, s in snaps.items()}
    print("filter of %d keys (%.1f %%): ps_snapshot_filter_new %.3f ms each" % (len(fs["1"]), 100 * frac, (time.perf_counter() - t) * 500), flush=True)
    for k in map(int, args.ks.split(",")):
        for d in ("1", "0"):
            leg("%.1f %% k=%d PS_FILTER_DRIVE=%s" % (100 * frac, k, d), snaps[d],
                lambda: snaps[d].query_batch_arrays(qs, sc, None, boosts, k, filter=fs[d], **kw), False)
    for d in ("1", "0"):
        leg("%.1f %% count PS_FILTER_DRIVE=%s" % (100 * frac, d), snaps[d], lambda: snaps[d].count_batch(qs, sc, boosts, filter=fs[d], **kw), True)
    for f in fs.values():
        f.close()
