"""Score-tiered scan copies (PS_DAAT_TIERS; ps_prep_kernels.hpp k_tier_*, k_prep_items, k_daat_small): the own stream of
k_daat_small reads a copy of every long list partitioned into tiers by a boost-free score key, and an item whose tiers cannot
reach the query's threshold is never read.  Rank-safe: tiers on == tiers off == the streaming kernel (PS_DAAT=0), bit for
bit, keys and scores, and == the oracle."""
import os
import random

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer
from emu import bits
from oracle import oracle as orc
from probly_search_amd import synth

pytestmark = pytest.mark.gpu

BOOSTS = ([1.0, 1.0], [0.5, 3.0], [2.0, 0.25])


def _set_tiers(L, on, min_len=None):
    """The minimum tiered length is an experiment knob read from the environment; any ps_set_option makes engines re-read."""
    if min_len is None:
        os.environ.pop("PS_DAAT_TIER_MIN", None)
    else:
        os.environ["PS_DAAT_TIER_MIN"] = str(min_len)
    L.ps_set_option(b"PS_DAAT_TIERS", on)


def _batch(snap, queries, boosts, K, F=2):
    snap.work_counters(reset=True)
    got = [[(r.key, bits(r.score)) for r in rs] for rs in snap.query_batch(queries, product_scorer("bm25"), None, boosts[:F], top_k=K)]
    return got, snap.work_counters(reset=True), snap.kernel_breakdown()["score_kernel"]


def _three_way(snap, o, queries, boosts, K, min_len, F=2, oracle_every=8, want="ps::k_daat_small", chunk=4096):
    """tiers on == off == streaming == oracle (every `oracle_every`-th query); returns the two work-counter sets.
    `chunk`: PS_DAAT_CHUNK, postings per item - small enough that the items of a short list fall inside its tiers."""
    L = psa.load()
    try:
        L.ps_set_option(b"PS_DAAT_CHUNK", chunk)
        _set_tiers(L, 1, min_len)
        on, w1, name = _batch(snap, queries, boosts, K, F)
        assert name.startswith(want), name
        _set_tiers(L, 0, min_len)
        off, w0, _ = _batch(snap, queries, boosts, K, F)
        assert on == off, (K, boosts, min_len, [i for i, (a, b) in enumerate(zip(on, off)) if a != b][:5])
        L.ps_set_option(b"PS_DAAT", 0)
        streamed, _, _ = _batch(snap, queries, boosts, K, F)
        L.ps_set_option(b"PS_DAAT", 1)
        assert streamed == on, (K, boosts, min_len)
        osc = oracle_scorer("bm25")
        for q, g in list(zip(queries, on))[::oracle_every]:
            exp = [(k, bits(s)) for k, s in o.query(q, osc, boosts[:F])[:K]]
            assert g == exp, (K, boosts, q, g[:3], exp[:3])
        return w1, w0
    finally:
        L.ps_set_option(b"PS_DAAT", 1)
        L.ps_set_option(b"PS_DAAT_CHUNK", 4096)
        _set_tiers(L, 1)  # (the defaults: tests/conftest.py does not know this knob)


@pytest.fixture(scope="module")
def corpus_pair():
    cfg = dict(synth.CONFIGS["C2"], n_docs=50_000, vocab=2_000)
    corpus = synth.Corpus(**cfg)
    p, o = synth.fill(psa.Index(2), corpus), synth.fill(orc.Index(2), corpus)
    return corpus, p, o, p.snapshot(device=0, headroom_pct=10)


@pytest.mark.parametrize("min_len", [4096, 300])
@pytest.mark.parametrize("K", [1, 10, 17, 64])
def test_tiers_change_work_not_results(corpus_pair, K, min_len):
    corpus, p, o, snap = corpus_pair
    queries = corpus.queries(64, 3, salt=123)
    L = psa.load()
    try:
        for dev_plan in (1, 0):
            L.ps_set_option(b"PS_DEVICE_PLAN", dev_plan)
            for boosts in BOOSTS:
                w1, w0 = _three_way(snap, o, queries, boosts, K, min_len)
                assert w1["postings_scanned"] <= w0["postings_scanned"], (K, boosts, w1, w0)
                if K <= 10 and boosts == [1.0, 1.0]:
                    assert w1["postings_scanned"] < w0["postings_scanned"], (K, w1["postings_scanned"], w0["postings_scanned"])
    finally:
        L.ps_set_option(b"PS_DEVICE_PLAN", 1)


def test_ties_across_a_tier_boundary():
    """Many duplicated documents: equal keys, equal scores, K cuts through runs of ties - the key-ascending tie-break decides."""
    rng = random.Random(3)
    shapes = [(["alpha"] * a + ["pad"] * pa, ["beta"] * b + ["alpha"] * c + ["fill"] * pb)
              for a, pa, b, c, pb in [(1, 2, 1, 0, 9), (2, 1, 0, 1, 20), (1, 5, 2, 2, 12), (3, 0, 1, 0, 30), (0, 3, 1, 1, 16), (1, 1, 0, 0, 40)]]
    p, o = psa.Index(2), orc.Index(2)
    for k in range(6000):
        f0, f1 = shapes[rng.randrange(len(shapes))]
        vals = [" ".join(f0), " ".join(f1 + (["gamma"] if k % 4 == 0 else []))]
        p.add_field_values(k, vals)
        o.add_document(k, vals)
    snap = p.snapshot(device=0)
    queries = ["alpha beta", "alpha gamma", "beta gamma alpha", "alpha fill", "gamma pad beta", "alpha", "beta pad", "fill gamma"] * 2
    for K in (3, 10, 64):
        for boosts in BOOSTS:
            w1, w0 = _three_way(snap, o, queries, boosts, K, 256, oracle_every=1, chunk=256)
            print("ties", K, boosts, w1["postings_scanned"], w0["postings_scanned"], w1["items_run"], w0["items_run"])
            if K <= 10 and boosts == [1.0, 1.0]:  # (the items are cut inside the tiers: whole tiers must have been dropped)
                assert w1["postings_scanned"] < w0["postings_scanned"], (K, w1["postings_scanned"], w0["postings_scanned"])


def test_degenerate_lists_and_one_field():
    """One field; `same`: tf 1 in a three-token field wherever it occurs - every posting has one key, the list is one tier;
    `edge`: exactly one posting over the minimum tiered length; `hot`: term frequencies 1..4 in fields of 4..12 tokens, keys
    spread over all tiers.  256-posting items, so items lie inside tiers and whole tiers are dropped."""
    n, min_len = 3000, 500
    p, o = psa.Index(1), orc.Index(1)
    rng = random.Random(9)
    n_edge = n_same = 0
    for k in range(n):
        if k % 3 != 2:
            words = ["same", "edge" if k <= 750 else "x%d" % (k % 11), "z%d" % (k % 5)]  # always three tokens
            n_same += 1
            n_edge += words[1] == "edge"
        else:
            words = ["hot"] * rng.randrange(1, 5) + ["y"] * rng.randrange(1, 6) + ["x%d" % (k % 11), "z%d" % (k % 5)]
        vals = [" ".join(words)]
        p.add_field_values(k, vals)
        o.add_document(k, vals)
    assert n_edge == min_len + 1 and n_same == 2000, (n_edge, n_same)
    snap = p.snapshot(device=0)
    queries = ["same hot", "edge hot", "same edge", "hot x3", "edge x1 z2", "same x4 hot", "hot", "edge", "same y", "hot z1 y"]
    for K in (1, 10, 64):
        w1, w0 = _three_way(snap, o, queries, [1.5], K, min_len, F=1, oracle_every=1, chunk=256)
        print("degenerate", K, w1["postings_scanned"], w0["postings_scanned"], w1["items_run"], w0["items_run"])
        if K <= 10:  # (`same`, `edge` and `hot` are tiered: the batch scans less with the copies than without)
            assert w1["postings_scanned"] < w0["postings_scanned"], (K, w1["postings_scanned"], w0["postings_scanned"])
    # the list of exactly the minimum length + 1 is tiered, one posting shorter it is not: with the minimum one above its
    # length nothing about `edge` alone may change
    e1, e0 = _three_way(snap, o, ["edge z1"] * 8, [1.5], 1, min_len + 2, F=1, oracle_every=8, chunk=256)
    t1, t0 = _three_way(snap, o, ["edge z1"] * 8, [1.5], 1, min_len, F=1, oracle_every=8, chunk=256)
    print("edge", e1["postings_scanned"], e0["postings_scanned"], t1["postings_scanned"], t0["postings_scanned"])
    assert t1["postings_scanned"] <= e1["postings_scanned"]


def test_mixed_batch_still_splits(corpus_pair):
    """One five-term query among three-term ones: the batch is split between the two kernels; the k_daat part reads originals."""
    corpus, p, o, snap = corpus_pair
    queries = corpus.queries(48, 3, salt=5)
    queries[7] = " ".join(q.split(" ")[0] for q in queries[:5])
    w1, w0 = _three_way(snap, o, queries, [1.0, 1.0], 10, 300, oracle_every=6, want="ps::k_daat_small<2, true, 4> + ps::k_daat<")
    assert w1["postings_scanned"] < w0["postings_scanned"], (w1["postings_scanned"], w0["postings_scanned"])  # (the small part is tiered)


def test_after_snapshot_update(corpus_pair):
    """(last: it mutates the module's index)  A delta changes every plane value: with tombstones or delta layers the own streams
    read the originals - removals only, then additions; tiers on == off == streaming == oracle."""
    corpus, p, o, snap = corpus_pair
    queries = corpus.queries(32, 3, salt=44)
    rng = random.Random(2)
    for k in rng.sample(range(50_000), 800):
        p.remove_document(k)
        o.remove_document(k)
    assert snap.update()["mode"] in (1, 2)
    _three_way(snap, o, queries, [1.0, 1.0], 10, 300, oracle_every=4, want="ps::k_daat")
    fresh = synth.Corpus(**dict(synth.CONFIGS["C2"], n_docs=400, vocab=2_000, seed=77))
    for keys, text, offsets in fresh.chunks():
        keys = keys + np.uint64(50_000)
        p.add_documents_flat(keys, text, offsets)
        o.add_documents_flat(keys, text, offsets)
    assert snap.update()["mode"] in (1, 2)
    _three_way(snap, o, queries, [0.5, 3.0], 10, 300, oracle_every=4, want="ps::k_daat")
