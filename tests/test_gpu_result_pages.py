"""Result pages (skip, top_k): k_deep_window behind the paged entry points, against the oracle's full result list
sliced [skip:skip + k], bit for bit.  Corpora and helpers are test_gpu_deep_topk.py's."""
from itertools import groupby

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer
from emu import bits
from oracle import oracle as orc
from probly_search_amd import dist as psd, synth
from test_gpu_deep_topk import BOOSTS, QUERIES, assert_same, build, corpus, expected  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
# inside the one-sided regime (skip + k <= 1024) | straddling 1024 | wholly beyond | a partial last page | at n | past n
PAGES = [(1, 10), (60, 10), (924, 100), (1000, 100), (1024, 1024), (1500, 64), (2990, 100), (3000, 10), (5000, 10)]


def device_page(snap, queries, boosts, skip, k, sc):
    text, offsets = synth.pack_queries(list(queries))
    B = len(queries)
    buf = psd._DeviceBuffer(psd.block_bytes(B, k))
    base = buf.ptr.value
    snap.query_batch_device_flat(text, offsets, sc, boosts, k, base, base + 8 * B * k, base + 16 * B * k, skip=skip)
    return psd.unpack_blocks(buf.to_host(), 1, B, k, [B])


@pytest.mark.parametrize("name", ["bm25", "zero_to_one"])
@pytest.mark.parametrize("skip,k", PAGES)
def test_regimes_and_entry_points(corpus, expected, skip, k, name):
    _, _, snap = corpus
    sc, exp = product_scorer(name), expected[name]
    assert {0, 1025, 3000} <= {len(e) for e in exp}  # the empty query; hi just above 1024 at (1000, 100); the longest run
    # 0: the page lies behind the run, 1: one-sided (hi <= 1024), 2: two-sided - over all pages and queries
    assert {0 if s >= len(e) else 1 if min(len(e), s + kk) <= 1024 else 2 for s, kk in PAGES for e in exp} == {0, 1, 2}
    batch = snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=k, skip=skip)
    device = device_page(snap, QUERIES, BOOSTS, skip, k, sc)
    for q, e, b, d in zip(QUERIES, exp, batch, device):
        assert_same(b, e[skip:skip + k], (name, skip, k, q, "query_batch"))
        assert_same(d, e[skip:skip + k], (name, skip, k, q, "device block"))
        assert_same(snap.query(q, sc, None, BOOSTS, top_k=k, skip=skip), e[skip:skip + k], (name, skip, k, q, "query"))
    assert snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=k, skip=0) == snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=k)


@pytest.fixture(scope="module", params=[1, 2], ids=lambda g: "20000-%dgroups" % g)
def tied(request):
    """test_gpu_deep_topk.py's two 20 000-document fixtures: one group of identical documents, or two interleaved
    groups of ~9 000 (each more than the LDS candidate buffer, at most half of the run) + 2 000 others."""
    n, groups = 20000, request.param
    docs = ["same word"] * n
    if groups == 2:
        docs = ["same word" if d % 20 < 9 else "same other thing" if d % 20 < 18 else "same" + " pad" * (3 + d % 7) for d in range(n)]
    for d, t in ((0, "same"), (n // 2, "same same"), (n - 1, "same word word word"), (7, "same other")):
        docs[d] = t
    text, offsets = synth.pack_queries(docs)
    keys = np.arange(n, dtype=np.uint64) * 2 + 10
    o, p = orc.Index(1), psa.Index(1)
    o.add_documents_flat(keys, text, offsets)
    p.add_documents_flat(keys, text, offsets)
    return groups, o, p.snapshot(device=0)


@pytest.mark.parametrize("name", ["bm25", "zero_to_one"])
@pytest.mark.parametrize("k", [65, 1024])
def test_ties_at_the_window_boundaries(tied, k, name):
    groups, o, snap = tied
    exp = o.query("same", oracle_scorer(name), [1.0])
    score = [bits(s) for _, s in exp]
    runs, at = [], 0  # (start, length) of the groups of equal scores, in rank order
    for _, g in groupby(score):
        runs.append((at, len(list(g))))
        at += runs[-1][1]
    big = [(s, ln) for s, ln in runs if ln > 8192]
    assert len(big) == groups and (groups == 1 or all(ln <= 20000 // 2 for _, ln in big))
    (a0, a_len), (b0, _) = big[0], big[-1]
    pages = {"inside": a0 + 2000, "group start": b0}
    # (a) both boundaries inside one group: the neighbours outside the window have the window's score
    assert score[pages["inside"] - 1] == score[pages["inside"] + k] and pages["inside"] + k < a0 + a_len
    # (c) the window starts at the first element of a group (and lies beyond rank 0)
    assert b0 > 0 and score[b0 - 1] != score[b0] == score[b0 + k - 1]
    if groups == 2:  # (b) from the first group into the second: both boundary bins are whole groups, larger than the LDS buffer
        pages["crossing"] = b0 - k // 2
        assert b0 == a0 + a_len and score[pages["crossing"]] == score[a0] != score[pages["crossing"] + k - 1] == score[b0]
    sc = product_scorer(name)
    for what, skip in pages.items():
        assert_same(snap.query_batch(["same", "word"], sc, None, [1.0], top_k=k, skip=skip)[0], exp[skip:skip + k], (what, skip, k, "query_batch"))
        assert_same(device_page(snap, ["same"], [1.0], skip, k, sc)[0], exp[skip:skip + k], (what, skip, k, "device block"))


def test_tombstones_are_never_on_a_page():
    o, p = build(1500, seed=11)
    snap = p.snapshot(device=0, tile_docs=256)
    removed = [3 * d + 1 for d in range(0, 1500, 10)]
    for key in removed:
        o.remove_document(key)
        p.remove_document(key)
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    for name in ("bm25", "zero_to_one"):
        sc = product_scorer(name)
        for q, b, d in zip(QUERIES, snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=100, skip=500),
                           device_page(snap, QUERIES, BOOSTS, 500, 100, sc)):
            exp = o.query(q, oracle_scorer(name), BOOSTS)[500:600]
            assert not {r.key for r in b} & set(removed)
            assert_same(b, exp, (name, q, "query_batch"))
            assert_same(d, exp, (name, q, "device block"))


def test_sliced_batch_equals_unsliced(corpus, expected, monkeypatch):
    monkeypatch.setenv("PS_FULL_BUDGET_MB", "0")  # read when the engine is created: every query is a slice of its own
    snap = corpus[1].snapshot(device=0, tile_docs=256)
    queries = (QUERIES * 3)[:40]
    sc = product_scorer("bm25")
    whole = corpus[2].query_batch(queries, sc, None, BOOSTS, top_k=128, skip=1200)
    for i, (b, d, w) in enumerate(zip(snap.query_batch(queries, sc, None, BOOSTS, top_k=128, skip=1200),
                                      device_page(snap, queries, BOOSTS, 1200, 128, sc), whole)):
        exp = expected["bm25"][i % len(QUERIES)][1200:1328]
        assert_same(w, exp, (i, "unsliced"))
        assert_same(b, exp, (i, "sliced query_batch"))
        assert_same(d, exp, (i, "sliced device block"))


def test_sharded_single_rank(corpus, expected):
    got = psd.query_batch_sharded(corpus[2], QUERIES, product_scorer("bm25"), BOOSTS, 100, skip=1100)
    for q, e, g in zip(QUERIES, expected["bm25"], got):
        assert_same(g, e[1100:1200], (q, "sharded"))


def test_bounds(corpus):
    _, _, snap = corpus
    sc = product_scorer("bm25")
    for k in (0, 1025):
        with pytest.raises(psa._lib.PsError):
            snap.query_batch(QUERIES[:3], sc, None, BOOSTS, top_k=k, skip=5)
        with pytest.raises(psa._lib.PsError):
            device_page(snap, QUERIES[:3], BOOSTS, 5, k, sc)
