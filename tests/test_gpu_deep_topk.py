"""Deep top-k (64 < k <= 1024): k_deep_select behind every query entry point, against the oracle's full result list
cut to k, bit for bit (the path moves no arithmetic: it only selects and orders what stage 1 scored)."""
import random

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer, run_device_planned
from emu import bits
from oracle import oracle as orc
from probly_search_amd import dist as psd, synth

pytestmark = pytest.mark.gpu
BOOSTS = [1.0, 1.5]
# document frequencies that put runs on every side of 65 / k / 1024 / the LDS candidate buffer
MARKS = {"ra": 40, "rb": 65, "rc": 90, "rd": 700, "re": 1024, "rf": 1025}
QUERIES = ["", "zzzz"] + sorted(MARKS) + ["fa", "fb fc", "ra rc", "f", "rd fa", "r"]


def assert_same(got, exp, ctx):
    got = [tuple(r) for r in got]
    assert [k for k, _ in got] == [k for k, _ in exp], (ctx, got[:5], exp[:5], len(got), len(exp))
    for (k, a), (_, b) in zip(got, exp):
        assert bits(a) == bits(b), (ctx, k, a.hex(), b.hex())


def build(n_docs, seed=7):
    """Two fields of a few filler words (fa..fh) + marker words with exact document frequencies -> (oracle, product)."""
    rng = random.Random(seed)
    fill = ["f" + c for c in "abcdefgh"]
    words = [[rng.choice(fill) for _ in range(rng.randint(1, 5))] for _ in range(n_docs)]
    for w, df in MARKS.items():
        for d in rng.sample(range(n_docs), min(df, n_docs)):
            words[d].insert(rng.randint(0, len(words[d])), w)
    o, p = orc.Index(2), psa.Index(2)
    for d, ws in enumerate(words):
        vals = [" ".join(ws), " ".join(rng.choice(fill) for _ in range(rng.randint(0, 3)))]
        o.add_document(3 * d + 1, vals)
        p.add_field_values(3 * d + 1, vals)
    return o, p


@pytest.fixture(scope="module")
def corpus():
    o, p = build(3000)
    return o, p, p.snapshot(device=0, tile_docs=256)


@pytest.fixture(scope="module")
def expected(corpus):
    o = corpus[0]
    return {name: [o.query(q, oracle_scorer(name), BOOSTS) for q in QUERIES] for name in ("bm25", "zero_to_one")}


@pytest.mark.parametrize("name", ["bm25", "zero_to_one"])
@pytest.mark.parametrize("k", [65, 100, 1000, 1024])
def test_entry_points_and_run_lengths(corpus, expected, k, name):
    _, _, snap = corpus
    sc, exp = product_scorer(name), expected[name]
    assert {0, 3000, *MARKS.values()} <= {len(e) for e in exp}  # runs of every class
    batch = snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=k)
    device = run_device_planned(snap, QUERIES, BOOSTS, k, sc)
    for q, e, b, d in zip(QUERIES, exp, batch, device):
        assert_same(b, e[:k], (name, k, q, "query_batch"))
        assert_same(d, e[:k], (name, k, q, "device block"))
        assert_same(snap.query(q, sc, None, BOOSTS, top_k=k), e[:k], (name, k, q, "query"))


def test_sharded_single_rank(corpus, expected):
    got = psd.query_batch_sharded(corpus[2], QUERIES, product_scorer("bm25"), BOOSTS, 100)
    for q, e, g in zip(QUERIES, expected["bm25"], got):
        assert_same(g, e[:100], (q, "sharded"))


@pytest.fixture(scope="module", params=[(1500, 1), (20000, 1), (20000, 2)], ids=lambda p: "%d-%dgroups" % p)
def tied(request):
    """N documents in one or two groups of identical ones around a few distinct ones, so the cut falls between equal
    scores.  One group of 20 000: the tie group is nearly the whole run and is filtered in place until the doc-id levels
    split it.  Two interleaved groups of ~9 000 + 2 000 others: the cut's tie group is more than the LDS candidate buffer
    and less than half of the run, so it is compacted into the global scratch and read back from there."""
    n, groups = request.param
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
    return n, groups, o, p.snapshot(device=0)


@pytest.mark.parametrize("name", ["bm25", "zero_to_one"])
@pytest.mark.parametrize("k", [65, 1024])
def test_ties_across_the_cut(tied, k, name):
    n, groups, o, snap = tied
    exp = o.query("same", oracle_scorer(name), [1.0])
    assert len(exp) == n and len({bits(s) for _, s in exp[5:k + 5]}) == 1  # the cut lies inside the block of equal scores
    tie_keys = [key for key, s in exp if bits(s) == bits(exp[k][1])]
    assert tie_keys == sorted(tie_keys)  # the lowest keys of the block win
    assert groups == 1 or 8192 < len(tie_keys) <= n // 2  # (8192 = k_deep_select's LDS candidate buffer)
    sc = product_scorer(name)
    assert_same(snap.query_batch(["same", "word"], sc, None, [1.0], top_k=k)[0], exp[:k], (n, k, name, "query_batch"))
    assert_same(run_device_planned(snap, ["same"], [1.0], k, sc)[0], exp[:k], (n, k, name, "device block"))


def test_tombstones_are_never_selected():
    o, p = build(1500, seed=11)
    snap = p.snapshot(device=0, tile_docs=256)
    removed = [3 * d + 1 for d in range(0, 1500, 10)]
    for key in removed:
        o.remove_document(key)
        p.remove_document(key)
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    for name in ("bm25", "zero_to_one"):
        sc = product_scorer(name)
        for q, b, d in zip(QUERIES, snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=100),
                           run_device_planned(snap, QUERIES, BOOSTS, 100, sc)):
            exp = o.query(q, oracle_scorer(name), BOOSTS)[:100]
            assert not {r.key for r in b} & set(removed)
            assert_same(b, exp, (name, q, "query_batch"))
            assert_same(d, exp, (name, q, "device block"))


def test_sliced_batch_equals_unsliced(corpus, expected, monkeypatch):
    monkeypatch.setenv("PS_FULL_BUDGET_MB", "0")  # read when the engine is created: every query is a slice of its own
    snap = corpus[1].snapshot(device=0, tile_docs=256)
    queries = (QUERIES * 3)[:40]
    sc = product_scorer("bm25")
    whole = corpus[2].query_batch(queries, sc, None, BOOSTS, top_k=128)
    for i, (b, d, w) in enumerate(zip(snap.query_batch(queries, sc, None, BOOSTS, top_k=128),
                                      run_device_planned(snap, queries, BOOSTS, 128, sc), whole)):
        exp = expected["bm25"][i % len(QUERIES)][:128]
        assert_same(w, exp, (i, "unsliced"))
        assert_same(b, exp, (i, "sliced query_batch"))
        assert_same(d, exp, (i, "sliced device block"))
    # full-result mode (every match; more than the deep path's 1024) over the same budget: the batch is halved down to
    # single queries, each sorted and downloaded on its own
    for name in ("bm25", "zero_to_one"):
        sc = product_scorer(name)
        for k in (0, 1025):
            for i, (b, w) in enumerate(zip(snap.query_batch(queries, sc, None, BOOSTS, top_k=k),
                                           corpus[2].query_batch(queries, sc, None, BOOSTS, top_k=k))):
                exp = expected[name][i % len(QUERIES)]
                exp = exp[:k] if k else exp
                assert_same(w, exp, (name, k, i, "unsliced full"))
                assert_same(b, exp, (name, k, i, "halved full"))


def test_bounds(corpus, expected):
    _, _, snap = corpus
    sc = product_scorer("bm25")
    for k in (0, 1025):
        with pytest.raises(psa._lib.PsError):
            run_device_planned(snap, QUERIES[:3], BOOSTS, k, sc)
    assert len(run_device_planned(snap, ["f"], BOOSTS, 1024, sc)[0]) == 1024
    for e, b in zip(expected["bm25"], snap.query_batch(QUERIES, sc, None, BOOSTS, top_k=1025)):
        assert_same(b, e[:1025], "host top-1025")
