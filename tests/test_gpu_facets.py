"""Facet counts (ps_snapshot_facet_counts_batch*: k_facet_counts and, behind the slow route, k_facet_runs) against a
np.bincount of the facet values of the oracle's full result list for the same index, scorer, boosts and query.  Keys are
0..N-1, so doc id == key; the corpus puts matching documents on the edges of the bitset's 64-document chunks, of its
32-bit words and of the 1024-document windows of PS_COUNT_WINDOW_LOG2 = 10.  Counts are integers: every comparison is
exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import probly_search_amd as psa
from adapters import oracle_scorer, product_scorer
from oracle import oracle as orc
from probly_search_amd import dist as psd, synth

pytestmark = pytest.mark.gpu
N, W = 3000, 1024
EINVAL, EUNSUPPORTED = psa._lib.PS_EINVAL, psa._lib.PS_EUNSUPPORTED
# route -> scorer, boosts, match mode, filtered.  fast kernel | its zero-boost instantiation | slow route (k_facet_runs) |
# fast kernel, boosts unread | slow route over k_conj's runs | fast kernel under the filter's bitmap
ROUTES = {"positive": ("bm25", [1.0, 1.5], "any", False), "zero boost": ("bm25", [1.0, 0.0], "any", False),
          "negative boost": ("bm25", [1.0, -0.5], "any", False), "zero_to_one": ("zero_to_one", [1.0, 1.0], "any", False),
          "match all": ("bm25", [1.0, 1.5], "all", False), "filter": ("bm25", [1.0, 1.5], "any", True)}
TERMS = {"chunk": [63, 64, 127, 128], "word": [31, 32, 95, 96], "win": [W - 1, W, W + 1, 2 * W - 1, 2 * W], "last": [N - 1],
         "oa": range(100, 200), "ob": range(150, 250),  # two overlapping lists
         "pre": range(300, 320), "prex": range(310, 330), "prexy": range(320, 340)}  # "pre" expands to three lists
QUERIES = ["", "nope", "chunk", "word", "win", "last", "all", "oa ob", "pre", "zf", "chunk win zf nope"]
ALLOWED = set(range(0, N, 5))


def fields(d):
    f0 = ["all"] + [t for t, ds in TERMS.items() if d in ds] + (["zf"] if 430 <= d < 480 else [])
    return [" ".join(f0), "zf" if 400 <= d < 450 else ""]  # 400..429 hold "zf" in field 1 only: no match under boost 0


def build():
    o, p = orc.Index(2), psa.Index(2)
    for d in range(N):
        o.add_document(d, fields(d))
        p.add_field_values(d, fields(d))
    return o, p


def facet_pairs(V):
    """d -> d % V, every 7th document without a value; key 64 twice (the larger value first), one unknown key."""
    keys = [64] + [d for d in range(N) if d % 7 != 3] + [N + 5]
    return keys, [V - 1] + [d % V for d in keys[1:-1]] + [0]


def matched(o, route, queries):
    """The keys of every query's full result list under `route`, restricted in plain Python where the route says so."""
    name, boosts, match, filtered = ROUTES[route]
    run = lambda q: [k for k, _ in o.query(q, oracle_scorer(name), boosts)]
    out = []
    for q in queries:
        keys = run(q)
        if match == "all":
            alone = [set(run(t)) for t in q.split()]
            keys = [k for k in keys if all(k in s for s in alone)] if alone else []
        out.append([k for k in keys if not filtered or k in ALLOWED])
    return out


@functools.lru_cache(maxsize=None)
def build_once():
    return build()


@functools.lru_cache(maxsize=None)
def matched_cached(route):
    return matched(build_once()[0], route, QUERIES)


def expected(keys_per_query, pairs, V):
    value = {}
    for k, v in zip(*pairs):
        value[k] = max(v, value.get(k, 0))
    return np.array([np.bincount([value[k] for k in keys if k in value], minlength=V) for keys in keys_per_query], np.uint64).reshape(-1, V)


def call_args(snap, route):
    name, boosts, match, filtered = ROUTES[route]
    return product_scorer(name), boosts, dict(match=match, filter=snap.filter(sorted(ALLOWED)) if filtered else None)


def snapshot(monkeypatch, w_log2):
    if w_log2:
        monkeypatch.setenv("PS_COUNT_WINDOW_LOG2", str(w_log2))  # read when the snapshot's engine is created
    return build_once()[1].snapshot(device=0, tile_docs=256)


@pytest.mark.parametrize("V", [1, 3, 64, 8192])  # one bin | 64 replicas | fewer replicas | the limit, the window capped
@pytest.mark.parametrize("w_log2", [8, 10, 19, None])  # 12 windows | 3 | wider than the corpus (and than the cap) | the rule
def test_windows_and_value_counts(monkeypatch, w_log2, V):
    snap = snapshot(monkeypatch, w_log2)
    sc, boosts, _ = call_args(snap, "positive")
    pairs = facet_pairs(V)
    facet = snap.facet(*pairs, n_values=V)
    assert (facet.n_values, len(facet)) == (V, len(set(pairs[0])) - 1)
    got = snap.facet_counts_batch(QUERIES, sc, boosts, facet)
    assert got.shape == (len(QUERIES), V) and got.dtype == np.uint64
    assert np.array_equal(got, expected(matched_cached("positive"), pairs, V))
    totals = snap.count_batch(QUERIES, sc, boosts)
    assert (got.sum(axis=1) <= totals).all() and got.sum() < totals.sum()
    every = snap.facet(range(N), [d % V for d in range(N)])  # n_values = max + 1
    assert every.n_values == min(V, N)
    assert np.array_equal(snap.facet_counts_batch(QUERIES, sc, boosts, every).sum(axis=1), totals)


@pytest.mark.parametrize("V", [3, 8192])
@pytest.mark.parametrize("route", ROUTES)
def test_routes(monkeypatch, route, V):
    snap = snapshot(monkeypatch, 10)
    sc, boosts, kw = call_args(snap, route)
    pairs = facet_pairs(V)
    facet = snap.facet(*pairs, n_values=V)
    got = snap.facet_counts_batch(QUERIES, sc, boosts, facet, **kw)
    assert np.array_equal(got, expected(matched_cached(route), pairs, V))
    assert (got.sum(axis=1) <= snap.count_batch(QUERIES, sc, boosts, **kw)).all()
    assert np.array_equal(snap.facet_counts_batch(QUERIES, sc, boosts, facet, **kw), got)  # a second call
    if route == "negative boost":  # field 1 holds nothing but "zf": for every other query the slow and the fast route agree
        rows = [i for i, q in enumerate(QUERIES) if "zf" not in q]
        fast = snap.facet_counts_batch(QUERIES, sc, ROUTES["positive"][1], facet)
        assert np.array_equal(got[rows], fast[rows]) and got[QUERIES.index("all")].sum() > 0


@pytest.mark.parametrize("route", ["positive", "negative boost"])
@pytest.mark.parametrize("B", [1, 300])
def test_device_form_batches_and_streams(monkeypatch, route, B):
    snap, V = snapshot(monkeypatch, 10), 64
    sc, boosts, _ = call_args(snap, route)
    pairs = facet_pairs(V)
    facet = snap.facet(*pairs, n_values=V)
    queries = [QUERIES[(i + 6) % len(QUERIES)] for i in range(B)]
    exp = expected(matched_cached(route), pairs, V)[[(i + 6) % len(QUERIES) for i in range(B)]]
    text, offsets = synth.pack_queries(queries)
    hip = psd._DeviceBuffer.hip()
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    for stream in (st.value, None):  # a caller stream | the NULL stream: synchronous
        buf = psd._DeviceBuffer(8 * B * V)
        buf.from_host(b"\xff" * (8 * B * V))  # counts the caller did not clear
        snap.facet_counts_batch_device_flat(text, offsets, sc, boosts, facet, buf.ptr.value, stream=stream)
        if stream:
            assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
        assert np.array_equal(np.frombuffer(buf.to_host(), np.uint64).reshape(B, V), exp), stream
    hip.hipStreamDestroy(st)


def test_tombstones_and_a_facet_from_before_the_update(monkeypatch):
    monkeypatch.setenv("PS_COUNT_WINDOW_LOG2", "10")
    (o, p), V = build(), 3
    snap = p.snapshot(device=0, tile_docs=256, headroom_pct=25)
    pairs = facet_pairs(V)
    old = snap.facet(*pairs, n_values=V)
    removed = [63, 64, W, N - 1, 150]
    for key in removed:
        o.remove_document(key)
        p.remove_document(key)
    assert snap.update()["mode"] == 1  # a delta: the postings stay, the alive bits go
    facet = snap.facet(*pairs, n_values=V)
    assert len(facet) == len(old) - sum(k in removed for k in set(pairs[0]))
    for route in ("positive", "negative boost"):
        sc, boosts, _ = call_args(snap, route)
        exp = expected(matched(o, route, QUERIES), pairs, V)
        assert np.array_equal(snap.facet_counts_batch(QUERIES, sc, boosts, facet), exp), route
        with pytest.raises(psa.PsError) as e:
            snap.facet_counts_batch(QUERIES, sc, boosts, old)
        assert e.value.status == EINVAL


def test_argument_errors():
    p = build_once()[1]
    snap, other, sc = p.snapshot(device=0, tile_docs=256), p.snapshot(device=0, tile_docs=256), product_scorer("bm25")
    for values, n_values, status in (([0, 3], 3, EINVAL), ([0, 1], 0, EINVAL), ([0, 1], 8193, EUNSUPPORTED)):
        with pytest.raises(psa.PsError) as e:
            snap.facet([1, 2], values, n_values=n_values)
        assert e.value.status == status, (values, n_values)
    empty = snap.facet([], [], n_values=4)  # n = 0: a valid facet that counts nothing
    assert len(empty) == 0 and not snap.facet_counts_batch(QUERIES, sc, [1.0, 1.0], empty).any()
    for bad in (other.facet([1], [0]), None):  # a facet of another snapshot | a null facet
        with pytest.raises(psa.PsError) as e:
            snap.facet_counts_batch(QUERIES, sc, [1.0, 1.0], bad)
        assert e.value.status == EINVAL
    L, facet = psa.load(), snap.facet([1], [0])
    desc, (b, nb), (qb, arr) = psa.index._scorer_desc(sc), psa.index._boosts([1.0, 1.0]), snap._pack_queries(QUERIES)
    out = np.zeros(len(qb), np.uint64)
    assert L.ps_snapshot_facet_counts_batch(snap._h, C.byref(desc), arr, len(qb), b, nb, None, None, facet._h, None) == EINVAL
    desc.kind = 3  # PS_SCORER_HOST_CALLBACKS: the snapshot entry points refuse it
    assert L.ps_snapshot_facet_counts_batch(snap._h, C.byref(desc), arr, len(qb), b, nb, None, None, facet._h, out.ctypes.data) == EINVAL
