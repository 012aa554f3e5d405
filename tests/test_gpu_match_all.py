"""Conjunctive queries (match="all", PS_MATCH_ALL: k_conj as stage 1 of every run consumer) against the oracle alone:
the oracle's result list of the query restricted to the documents in its result list of every non-empty token queried
by itself - keys and score bits, exactly.  Keys are 0..N-1, so doc id == key.  PS_CONJ_CHUNK = 64 cuts a driver list of
more than 64 postings into several items: "wide all" is driven by "wide" (2000 postings, 32 items, survivors on every
chunk edge), "oa" and "zf" drive two items each; in "wide edge" the driver is "edge" and its survivors sit on the chunk
edges of the list that is searched.  "pre" and "pre all" have a driver term of four lists that share documents (the
ownership rule: every document once).  PS_CONJ_LISTS = 2 takes the sub-ranges of a query's lists two at a time, so the
five entries of "pre prez" and "pre all" cross block edges in both phases."""
import ctypes as C

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer
from oracle import oracle as orc
from probly_search_amd import dist as psd, synth
from test_gpu_deep_topk import assert_same

pytestmark = pytest.mark.gpu
N = 6000
ROUTES = {"positive": [1.0, 1.5], "zero boost": [1.0, 0.0], "negative boost": [1.0, -0.5]}
WIDE = range(1, N, 3)  # 2000 postings
TERMS = {"wide": WIDE, "edge": [WIDE[i] for i in (63, 64, 127, 128, 1999)], "oa": range(100, 200), "ob": range(150, 250),
         "oc": range(180, 280), "prez": range(320, 360), "gap": [5, 5990], "dead": [7, 1024, 5998]}
QUERIES = ["", "nope", "oa", "oa ob", "oa ob oc", "oa oa", "oa nope", "pre oa", "pre prez", "wide edge", "gap all",
           "all wide oa", "zf all", "dead all", "pre", "pre all", "wide all"]
SIZES = [0, 0, 100, 50, 20, 100, 0, 0, 40, 5, 2, 34, 80, 3, 60, 60, 2000]  # under positive boosts


def values(d):
    f0 = ["all"] + [t for t, ds in TERMS.items() if d in ds]
    if 300 <= d < 340:
        f0 += ["pre", "prex", "prexy"]
    if 430 <= d < 480:
        f0.append("zf")
    return [" ".join(f0), "zf" if 400 <= d < 450 else ""]  # 400..429 hold "zf" in field 1 only


def build():
    o, p = orc.Index(2), psa.Index(2)
    for d in range(N):
        o.add_document(d, values(d))
        p.add_field_values(d, values(d))
    return o, p


@pytest.fixture(scope="module")
def corpus():
    return build()


def expected(o, boosts):
    sc, out = oracle_scorer("bm25"), []
    for q in QUERIES:
        toks = [t for t in q.split(" ") if t]
        keep = set.intersection(*[{k for k, _ in o.query(t, sc, boosts)} for t in toks]) if toks else set()
        out.append([r for r in o.query(q, sc, boosts) if r[0] in keep])
    return out


def device_block(snap, sc, boosts, k):
    text, offsets = synth.pack_queries(QUERIES)
    B = len(QUERIES)
    buf = psd._DeviceBuffer(psd.block_bytes(B, k))
    base = buf.ptr.value
    snap.query_batch_device_flat(text, offsets, sc, boosts, k, base, base + 8 * B * k, base + 16 * B * k, match="all")
    return psd.unpack_blocks(buf.to_host(), 1, B, k, [B])


def check(snap, o, boosts, ctx):
    sc, exp = product_scorer("bm25"), expected(o, boosts)
    calls = {"top_k=0": (snap.query_batch(QUERIES, sc, None, boosts, top_k=0, match="all"), slice(None)),
             "top_k=10": (snap.query_batch(QUERIES, sc, None, boosts, top_k=10, match="all"), slice(10)),
             "top_k=100": (snap.query_batch(QUERIES, sc, None, boosts, top_k=100, match="all"), slice(100)),
             "page": (snap.query_batch(QUERIES, sc, None, boosts, top_k=10, skip=5, match="all"), slice(5, 15)),
             "device block": (device_block(snap, sc, boosts, 10), slice(10))}
    for name, (got, cut) in calls.items():
        for q, g, e in zip(QUERIES, got, exp):
            assert_same(g, e[cut], (ctx, name, q))
    assert_same(snap.query("all wide oa", sc, None, boosts, match="all"), exp[QUERIES.index("all wide oa")], (ctx, "query"))
    assert snap.count_batch(QUERIES, sc, boosts, match="all").tolist() == [len(e) for e in exp], (ctx, "count")
    return exp


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("chunk,lists", [(64, None), (None, None), (64, 2)])
def test_routes_and_chunk_edges(corpus, monkeypatch, route, chunk, lists):
    o, p = corpus
    for knob, v in (("PS_CONJ_CHUNK", chunk), ("PS_CONJ_LISTS", lists)):
        if v:
            monkeypatch.setenv(knob, str(v))  # read when the snapshot's engine is created
    snap = p.snapshot(device=0, tile_docs=256)
    exp = check(snap, o, ROUTES[route], (route, chunk, lists))
    if route == "positive":  # what the corpus was built to show
        assert [len(e) for e in exp] == SIZES
    else:
        assert len(exp[QUERIES.index("zf all")]) == 50  # 400..429 score None in the field whose boost is not positive
    check(snap, o, ROUTES[route], (route, chunk, lists, "second call"))
    sc = product_scorer("bm25")
    default = snap.query_batch(QUERIES, sc, None, ROUTES[route], top_k=10)
    assert snap.query_batch(QUERIES, sc, None, ROUTES[route], top_k=10, match="any") == default
    assert snap.count_batch(QUERIES, sc, ROUTES[route], match="any").tolist() == snap.count_batch(QUERIES, sc, ROUTES[route]).tolist()


def test_tombstones_and_deltas(monkeypatch):
    monkeypatch.setenv("PS_CONJ_CHUNK", "64")
    monkeypatch.setenv("PS_CONJ_LISTS", "2")
    o, p = build()
    snap = p.snapshot(device=0, tile_docs=256, headroom_pct=25)

    def both(fn):
        fn(o)
        fn(p)

    for key in (*TERMS["dead"], 160):
        both(lambda ix: ix.remove_document(key))
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    for route, boosts in ROUTES.items():
        exp = check(snap, o, boosts, (route, "removed"))
        assert (len(exp[QUERIES.index("dead all")]), len(exp[QUERIES.index("oa ob")])) == (0, 49)
    for d in range(N, N + 70):
        o.add_document(d, ["all oa ob pre fresh", ""])
        p.add_field_values(d, ["all oa ob pre fresh", ""])
    assert snap.update()["mode"] == 1 and snap.info()["delta_layers"] > 0
    for route, boosts in ROUTES.items():
        assert len(check(snap, o, boosts, (route, "delta layers"))[QUERIES.index("oa ob")]) == 119
    both(lambda ix: ix.remove_document(N + 3))  # a tombstone in a delta layer
    o.add_document(1024, values(1024))  # a key removed and added again
    p.add_field_values(1024, values(1024))
    snap.update()
    for route, boosts in ROUTES.items():
        # (the re-added key stays in the reference's removed set until a vacuum: "dead all" is still empty)
        assert len(check(snap, o, boosts, (route, "key added again"))[QUERIES.index("oa ob")]) == 118


def test_errors(corpus):
    _, p = corpus
    snap, L, sc = p.snapshot(device=0, tile_docs=256), psa.load(), product_scorer("bm25")
    with pytest.raises(psa._lib.PsError) as e:
        snap.query_batch(QUERIES, product_scorer("zero_to_one"), None, [1.0, 1.0], top_k=10, match="all")
    assert e.value.status == psa._lib.PS_EUNSUPPORTED
    assert len(snap.query(" ".join(["all"] * 64), sc, None, [1.0, 1.0], top_k=3, match="all")) == 3  # 64 terms: the most
    with pytest.raises(psa._lib.PsError) as e:
        snap.query(" ".join(["all"] * 65), sc, None, [1.0, 1.0], top_k=3, match="all")
    assert e.value.status == psa._lib.PS_EUNSUPPORTED
    with pytest.raises(ValueError):
        snap.query_batch(QUERIES, sc, None, [1.0, 1.0], top_k=10, match="some")
    desc, (b, nb), (qb, arr) = psa.index._scorer_desc(sc), psa.index._boosts([1.0, 1.0]), snap._pack_queries(QUERIES)
    desc.match_mode = 2
    out = np.zeros(len(qb), np.uint64)
    st = C.c_void_p(snap._h.value)
    assert L.ps_snapshot_count_batch(st, C.byref(desc), arr, len(qb), b, nb, None, None, out.ctypes.data) == psa._lib.PS_EINVAL
    text, offsets = synth.pack_queries(QUERIES * 2)  # enough queries for the device planner to take the batch
    assert snap.plan_ahead_flat(text, offsets, sc, [1.0, 1.0], match="any")
    assert not snap.plan_ahead_flat(text, offsets, sc, [1.0, 1.0], match="all")
