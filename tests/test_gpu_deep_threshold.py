"""Thresholded stage 1 of deep top-k and result pages (k_deep_threshold): the answers stay the oracle's, bit for bit, and
work_counters()["run_results"], counted on the device, is exactly what the oracle's full lists predict for a sample of
PS_DEEP_SAMPLE_RUNS runs of 256 documents.  Corpora and helpers are test_gpu_deep_topk.py's and test_gpu_result_pages.py's."""
import numpy as np
import pytest

from adapters import oracle_scorer, product_scorer, run_device_planned
from emu import bits
from oracle import oracle as orc
import probly_search_amd as psa
from probly_search_amd import synth
from test_gpu_deep_topk import BOOSTS, assert_same, build
from test_gpu_result_pages import device_page

pytestmark = pytest.mark.gpu
# a filler word | two words | a prefix that expands | 40 matches (< hi) | exactly 65 | nothing | a repeated term (k_z21 takes it)
QUERIES = ["fa", "fb fc", "f", "ra", "rb", "", "fa fa"]


def snapshot(monkeypatch, index, sample_runs):
    monkeypatch.setenv("PS_TILES_PER_RUN", "1")  # both are read when the snapshot's engine is created
    monkeypatch.setenv("PS_DEEP_SAMPLE_RUNS", str(sample_runs))
    return index.snapshot(device=0, tile_docs=256)


def run_length(full, hi, first_key_outside):
    """Elements stage 1 leaves for a query whose every match is `full`, the sample being the keys below first_key_outside."""
    sample = sorted((bits(s) for k, s in full if k < first_key_outside), reverse=True)  # (scores >= 0: bits order like numbers)
    if len(sample) < hi:
        return len(full)
    return len(sample) + sum(1 for k, s in full if k >= first_key_outside and bits(s) >= sample[hi - 1])


def check(snap, exp, queries, boosts, sc, skip, k, want_runs, ctx):
    """query_batch and the device block against exp[skip : skip + k]; run_results of either call == want_runs."""
    snap.work_counters(reset=True)
    batch = snap.query_batch(queries, sc, None, boosts, top_k=k, skip=skip)
    assert snap.work_counters(reset=True)["run_results"] == want_runs, ctx
    device = device_page(snap, queries, boosts, skip, k, sc) if skip else run_device_planned(snap, queries, boosts, k, sc)
    assert snap.work_counters(reset=True)["run_results"] == want_runs, ctx
    for q, e, b, d in zip(queries, exp, batch, device):
        assert_same(b, e[skip:skip + k], (ctx, q, "query_batch"))
        assert_same(d, e[skip:skip + k], (ctx, q, "device block"))


@pytest.fixture(scope="module")
def corpus():
    o, p = build(3000)
    return o, p, {name: [o.query(q, oracle_scorer(name), BOOSTS) for q in QUERIES] for name in ("bm25", "zero_to_one")}


@pytest.mark.parametrize("name", ["bm25", "zero_to_one"])
@pytest.mark.parametrize("k,skip", [(65, 0), (1024, 0), (10, 100), (100, 1000)])
@pytest.mark.parametrize("sample_runs", [1, 4, 11])
def test_pages_and_run_lengths(corpus, monkeypatch, sample_runs, k, skip, name):
    _, p, expected = corpus
    exp = expected[name]
    assert [len(e) for e in exp[3:6]] == [40, 65, 0] and len(exp[0]) > 1024
    want = [run_length(e, skip + k, 3 * 256 * sample_runs + 1) for e in exp]
    if (k, skip, sample_runs) == (65, 0, 4):  # the threshold really prunes: it is not +0.0 everywhere
        # (BM25: 583 of 1278; zero_to_one's few distinct scores tie widely at thr and are all kept: 667, no filler word gets below half)
        assert want[0] < (len(exp[0]) // 2 if name == "bm25" else len(exp[0]) * 11 // 20)
    check(snapshot(monkeypatch, p, sample_runs), exp, QUERIES, BOOSTS, product_scorer(name), skip, k, sum(want), (name, k, skip, sample_runs))


def test_ties_at_the_threshold(monkeypatch):
    """Every repeat of one document ties at thr: >= keeps them all (the one longer document is dropped), the lowest keys win."""
    n = 1500
    docs = ["same word"] * n
    for d, t in ((0, "same"), (n // 2, "same same"), (n - 1, "same word word word"), (7, "same other")):
        docs[d] = t
    text, offsets = synth.pack_queries(docs)
    keys = np.arange(n, dtype=np.uint64) * 2 + 10
    o, p = orc.Index(1), psa.Index(1)
    o.add_documents_flat(keys, text, offsets)
    p.add_documents_flat(keys, text, offsets)
    snap = snapshot(monkeypatch, p, 1)
    for name in ("bm25", "zero_to_one"):
        exp = o.query("same", oracle_scorer(name), [1.0])
        want = run_length(exp, 65, 2 * 256 + 10)
        assert len(exp) == n and len({bits(s) for _, s in exp[5:70]}) == 1 and want == n - 1
        check(snap, [exp], ["same"], [1.0], product_scorer(name), 0, 65, want, name)


def test_tombstones_are_not_sampled(monkeypatch):
    o, p = build(1500, seed=11)
    snap = snapshot(monkeypatch, p, 2)
    for d in range(0, 1500, 10):
        o.remove_document(3 * d + 1)
        p.remove_document(3 * d + 1)
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    for name in ("bm25", "zero_to_one"):
        exp = [o.query(q, oracle_scorer(name), BOOSTS) for q in QUERIES]
        check(snap, exp, QUERIES, BOOSTS, product_scorer(name), 0, 100, sum(run_length(e, 100, 3 * 256 * 2 + 1) for e in exp), name)


def test_scores_that_may_be_negative_are_not_thresholded(corpus, monkeypatch):
    o, p, _ = corpus
    exp = [o.query(q, oracle_scorer("bm25"), [1.0, -0.5]) for q in QUERIES]
    check(snapshot(monkeypatch, p, 4), exp, QUERIES, [1.0, -0.5], product_scorer("bm25"), 0, 65, sum(len(e) for e in exp), "gate")
