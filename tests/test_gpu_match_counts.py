"""Exact total match counts (ps_snapshot_count_batch*, k_count_matches and the slow route behind it) against the length
of the oracle's full result list for the same index, scorer, boosts and query, cross-checked with len() of this
library's own top_k = 0 answer.  Keys are 0..N-1, so doc id == key and the corpus below puts matching documents on the
bitset-word and window edges of PS_COUNT_WINDOW_LOG2 = 10 (three windows of 1024 documents)."""
import ctypes as C

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer
from oracle import oracle as orc
from probly_search_amd import dist as psd, synth

pytestmark = pytest.mark.gpu
N, W = 3000, 1024
# fast kernel | its zero-boost instantiation (twice: "all" lives in field 0 only) | slow route | fast kernel, boosts unread
ROUTES = {"positive": ("bm25", [1.0, 1.5]), "zero boost": ("bm25", [1.0, 0.0]), "first boost zero": ("bm25", [0.0, 2.0]),
          "negative boost": ("bm25", [1.0, -0.5]), "zero_to_one": ("zero_to_one", [1.0, 1.0])}
TERMS = {"edge": [31, 32, 63, 64, W - 1, W, W + 1, 2 * W - 1, 2 * W, N - 1],  # w*32-1, w*32, W-1, W, W+1, the last document
         "endw": range(W - 24, W),              # a list that ends exactly at a window edge
         "gap": [5, 2 * W + 400],               # no posting in the middle window
         "oa": range(100, 200), "ob": range(150, 250), "oc": range(180, 280),  # documents in two and three lists
         "dead": [7, W, N - 2]}                 # every document of it is removed in the tombstone test
QUERIES = ["", "nope", "edge", "endw", "gap", "oa ob", "oa ob oc", "oa oa", "pre", "zf", "all", "edge gap zf nope", "dead"]
EDGE_KEYS = sorted({31, N - 1, W - 1, W, 100, 279, 5, 300, 449, *TERMS["dead"]})  # list heads, tails, window edges


def values(d):
    f0 = ["all"] + [t for t, ds in TERMS.items() if d in ds]
    if 300 <= d < 340:
        f0 += ["pre", "prex", "prexy"]  # "pre" expands to three lists holding the same documents
    if 430 <= d < 480:
        f0.append("zf")
    return [" ".join(f0), "zf" if 400 <= d < 450 else ""]  # 400..429 hold "zf" in field 1 only: not a match under boost 0


@pytest.fixture(scope="module")
def corpus():
    o, p = orc.Index(2), psa.Index(2)
    for d in range(N):
        o.add_document(d, values(d))
        p.add_field_values(d, values(d))
    return o, p


def oracle_totals(o, route, queries=QUERIES):
    name, boosts = ROUTES[route]
    return [len(o.query(q, oracle_scorer(name), boosts)) for q in queries]


def device_totals(snap, queries, sc, boosts, stream=None):
    text, offsets = synth.pack_queries(list(queries))
    buf = psd._DeviceBuffer(8 * len(queries))
    buf.from_host(b"\xff" * (8 * len(queries)))  # totals the caller did not clear
    snap.count_batch_device_flat(text, offsets, sc, boosts, buf.ptr.value, stream=stream)
    if stream:
        assert psd._DeviceBuffer.hip().hipStreamSynchronize(C.c_void_p(stream)) == 0
    return np.frombuffer(buf.to_host(), np.uint64).tolist()


def check(snap, o, route, ctx):
    name, boosts = ROUTES[route]
    sc, exp = product_scorer(name), oracle_totals(o, route)
    assert snap.count_batch(QUERIES, sc, boosts).tolist() == exp, (route, ctx, "host")
    assert device_totals(snap, QUERIES, sc, boosts) == exp, (route, ctx, "device")
    assert [len(r) for r in snap.query_batch(QUERIES, sc, None, boosts, top_k=0)] == exp, (route, ctx, "top_k = 0")
    return exp


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("w_log2", [8, 10, 19, None])  # 12 windows | 3 | wider than the corpus | the engine's own rule
def test_routes_windows_and_edges(corpus, monkeypatch, route, w_log2):
    o, p = corpus
    if w_log2:
        monkeypatch.setenv("PS_COUNT_WINDOW_LOG2", str(w_log2))  # read when the snapshot's engine is created
    snap = p.snapshot(device=0, tile_docs=256)
    exp = check(snap, o, route, w_log2)
    if route == "positive":  # what the corpus was built to show
        got = dict(zip(QUERIES, exp))
        assert (got[""], got["nope"], got["edge"], got["endw"], got["gap"], got["all"]) == (0, 0, 10, 24, 2, N)
        assert (got["oa ob"], got["oa ob oc"], got["oa oa"], got["pre"], got["zf"]) == (150, 180, 100, 40, 80)
    if route == "zero boost":
        assert exp[QUERIES.index("zf")] == 50  # 400..429 hold it in the boost-0 field only
    check(snap, o, route, (w_log2, "second call"))


@pytest.mark.parametrize("route", ["positive", "zero boost", "negative boost"])
@pytest.mark.parametrize("B", [1, 7, 8, 300])
def test_batch_sizes_and_streams(corpus, monkeypatch, route, B):
    o, p = corpus
    monkeypatch.setenv("PS_COUNT_WINDOW_LOG2", "10")
    snap = p.snapshot(device=0, tile_docs=256)
    name, boosts = ROUTES[route]
    sc = product_scorer(name)
    one = oracle_totals(o, route)
    queries = [QUERIES[(i + 2) % len(QUERIES)] for i in range(B)]
    exp = [one[(i + 2) % len(QUERIES)] for i in range(B)]
    hip = psd._DeviceBuffer.hip()
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    assert snap.count_batch(queries, sc, boosts).tolist() == exp
    assert device_totals(snap, queries, sc, boosts, stream=st.value) == exp  # a caller stream
    assert device_totals(snap, queries, sc, boosts) == exp                   # the NULL stream: synchronous
    hip.hipStreamDestroy(st)


def test_tombstones_deltas_and_vacuum(monkeypatch):
    monkeypatch.setenv("PS_COUNT_WINDOW_LOG2", "10")
    o, p = orc.Index(2), psa.Index(2)
    for d in range(N):
        o.add_document(d, values(d))
        p.add_field_values(d, values(d))
    snap = p.snapshot(device=0, tile_docs=256, headroom_pct=25)

    def both(fn):
        fn(o)
        fn(p)

    for key in EDGE_KEYS:
        both(lambda ix: ix.remove_document(key))
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    for route in ROUTES:
        assert check(snap, o, route, "removed")[QUERIES.index("dead")] == 0
    for d in range(N, N + 70):  # delta layers: appended documents, the last one in a fourth window
        vals = ["all edge oa pre fresh", "zf" if d % 2 else ""]
        o.add_document(d, vals)
        p.add_field_values(d, vals)
    both(lambda ix: ix.remove_document(150))
    assert snap.update()["mode"] == 1 and snap.info()["delta_layers"] > 0
    for route in ROUTES:
        check(snap, o, route, "delta layers")
    both(lambda ix: ix.remove_document(N + 3))  # a tombstone in a delta layer
    o.add_document(W, values(W))  # a key removed and added again
    p.add_field_values(W, values(W))
    snap.update()
    for route in ROUTES:
        check(snap, o, route, "key added again")
    both(lambda ix: ix.vacuum())
    snap.update()
    for route in ROUTES:
        check(snap, o, route, "vacuum")


def test_argument_errors_and_keyed_index(corpus):
    _, p = corpus
    snap, L = p.snapshot(device=0, tile_docs=256), psa.load()
    sc = product_scorer("bm25")
    with pytest.raises(IndexError):  # bm25.rs:85 would panic
        snap.count_batch(QUERIES, sc, [1.0])
    desc, (b, nb), (qb, arr) = psa.index._scorer_desc(sc), psa.index._boosts([1.0, 1.0]), snap._pack_queries(QUERIES)
    out = np.zeros(len(qb), np.uint64)
    st = C.c_void_p(snap._h.value)
    assert L.ps_snapshot_count_batch(st, C.byref(desc), arr, len(qb), b, nb, None, None, None) == psa._lib.PS_EINVAL
    assert L.ps_snapshot_count_batch(None, C.byref(desc), arr, len(qb), b, nb, None, None, out.ctypes.data) == psa._lib.PS_EINVAL
    assert L.ps_snapshot_count_batch(st, C.byref(desc), None, len(qb), b, nb, None, None, out.ctypes.data) == psa._lib.PS_EINVAL
    assert L.ps_snapshot_count_batch_device_flat(st, C.byref(desc), None, None, 3, b, nb, None, None, None, None) == psa._lib.PS_EINVAL
    desc.kind = 3  # PS_SCORER_HOST_CALLBACKS: the snapshot entry points refuse it
    assert L.ps_snapshot_count_batch(st, C.byref(desc), arr, len(qb), b, nb, None, None, out.ctypes.data) == psa._lib.PS_EINVAL
    with pytest.raises(psa._lib.PsError) as e:
        p.snapshot(device=-1).count_batch(QUERIES, sc, [1.0, 1.0])
    assert e.value.status == 5  # PS_ENODEVICE
    k = psa.keys.KeyedIndex(1)
    for key, text in (("u-1", "red fox"), ("u-2", "red"), ("u-3", "blue")):
        k.add_field_values(key, [text])
    assert k.snapshot(device=0).count_batch(["red", "fox blue", "green"], sc, [1.0]).tolist() == [2, 2, 0]
