// ps_kernels_conj.hpp — conjunctive ("match all") queries: Kj k_conj, an intersect-and-score stage 1.  It fills the
// same per-query runs of (doc, f64 score) behind full_off / full_cnt that full-result mode's k_score fills, so that
// everything behind stage 1 (k_deep_select, k_deep_window, k_count_copy, the full-result sort) serves it unchanged.
//
// A document is a result iff it is alive and every non-empty query term gave it Some(score) through one of the
// term's lists (expansions, version layers, delta layers); its score is max_score_merger's over ALL of the query's
// entries in plan order (query.rs:61-89,150-164) - the OR query's bits.
//
// The driver term of a query is the one with the fewest postings.  A work item is a chunk of at most CONJ_NT
// postings of one list of the driver term, one workgroup per item, one driver posting per lane:
//   ranges   the chunk spans the doc ids [first, last]; of every entry of the query only the postings inside that
//            span can matter - two wave-cooperative 64-ary searches per entry (count::lower_bound), one wave per
//            entry, the sub-ranges parked in LDS, CONJ_LISTS entries at a time.  A query of up to CONJ_LISTS
//            entries - nearly all - has its ranges found once, in plan order, for both phases; a longer one (a short
//            prefix owns any number of lists) is taken a block at a time: phase A's blocks follow the host's `order`,
//            phase B finds the ranges again in plan order, and only in the items that have survivors;
//   phase A  membership on doc ids alone, term by term in ascending total length (the host's order): a sub-range
//            of up to CONJ_STAGE ids is staged in LDS with 16-byte loads and binary-searched there by every lane
//            that still needs the term - not staged at all when no lane of the workgroup does -, a longer one is
//            searched in global memory; a lane that found its document skips the term's other lists; after a term
//            the lanes without it are dead, and a workgroup without a live lane ends.  Ownership: a document that
//            also occurs in an EARLIER list (plan order) of the driver term belongs to that list's item and is
//            dropped here, so every document is emitted once;
//   compact  survivors are packed into an LDS array by a ballot prefix: phase B has full lanes;
//   phase B  a lane takes one survivor and walks all entries in plan order: binary search in the entry's sub-range,
//            tf / field length through the packed words (tfl_exact), s = sum_x ((tfn * idf) * boost_x) * eb in the
//            order and association of k_score (ps_kernels_score.hpp, score_trip), Some iff s > 0, the merger rule
//            with the lane's "last query term that visited me" word, and one bit per query term that gave Some.
//            Membership was necessary, not sufficient (a posting may score None under a zero or negative boost):
//            only a document whose bit set is full is appended to the run (one atomic per wave).
// Integer searches and a handful of f64 operations per survivor: nothing is multiplied in bulk, no MFMA applies.
#pragma once
#include "ps_kernels_common.hpp"
#include "ps_kernels_count.hpp"
#include "ps_kernels_score.hpp"

namespace ps {

constexpr int CONJ_NT = 256;                // threads per item == most driver postings per item
constexpr int CONJ_WAVES = CONJ_NT / WAVE;
constexpr uint32_t CONJ_CHUNK = CONJ_NT;    // driver postings per item (PS_CONJ_CHUNK: 1..CONJ_NT)
constexpr uint32_t CONJ_LISTS = 1024;       // plan entries whose sub-ranges wait in LDS at a time (PS_CONJ_LISTS: 1..CONJ_LISTS)
constexpr uint32_t CONJ_STAGE = 4096;       // doc ids of a sub-range staged in LDS; a longer one is searched in global memory
constexpr uint32_t CONJ_MAX_TERMS = 64;     // non-empty terms of a match-all query: one bit each in a lane's u64

struct ConjItem { uint32_t q, entry, begin, count; };  // `count` postings from `begin` of plan entry `entry` (driver term of query q)

struct ConjParams {
  const uint32_t* order;     // [n_plan_entries] per query (at qbeg[q]): its entries, the driver term's first, then term by term in ascending total length
  const uint32_t* n_terms;   // [B] non-empty terms of the query
  const ConjItem* items;     // [grid]
  unsigned long long* run_results;  // ps_work_counters::run_results when no select kernel follows to count the runs; else null
  uint32_t lists;            // entries per block of ranges, 1..CONJ_LISTS
};

namespace conj {

// Position of `d` in the ascending ids a[lo, hi), or hi when it is not there.
template <typename I>
__device__ __forceinline__ I find(const uint32_t* a, I lo, const I hi, const uint32_t d) {
  I l = lo, h = hi;
  while (l < h) {
    const I mid = l + ((h - l) >> 1);
    if (a[mid] < d) l = mid + 1; else h = mid;
  }
  return (l < hi && a[l] == d) ? l : hi;
}

// doc[beg, end) -> stage[0, end - beg) by the whole workgroup: whole 16-byte vectors, the ragged ends element by
// element (a vector load never leaves the sub-range, so it never leaves the plane).
__device__ __forceinline__ void stage_ids(const uint32_t* doc, uint32_t* stage, const uint64_t beg, const uint64_t end, const int tid) {
  const uint64_t v0 = beg >> 2, v1 = (end + 3) >> 2;
  const uint4* doc4 = reinterpret_cast<const uint4*>(doc);
  for (uint64_t v = v0 + (uint64_t)tid; v < v1; v += CONJ_NT) {
    const uint64_t p = v << 2;
    if (p >= beg && p + 4 <= end) {
      const uint4 x = doc4[v];
      uint32_t* s = stage + (p - beg);
      s[0] = x.x; s[1] = x.y; s[2] = x.z; s[3] = x.w;
    } else {
      for (uint64_t i = p < beg ? beg : p; i < p + 4 && i < end; ++i) stage[i - beg] = doc[i];
    }
  }
}

// The sub-ranges inside the doc ids [first, last] of `cn` entries into slots 0 .. cn - 1, one wave per entry, between
// two barriers (nobody still reads the block that goes, everybody sees the one that comes).  The entries are
// ids[0 .. cn) when `ids` is given, else from + 0 .. from + cn - 1.  Every thread of the workgroup calls.
__device__ __forceinline__ void ranges(const KParams& p, uint32_t* r_beg, uint32_t* r_end, const uint32_t* ids, const uint32_t from,
                                       const uint32_t cn, const uint32_t first, const uint32_t last) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  __syncthreads();
  for (uint32_t i = (uint32_t)wave; i < cn; i += CONJ_WAVES) {
    const ps_plan_entry e = p.plan[ids ? ids[i] : from + i];
    const uint64_t lo = e.post_off, hi = e.post_off + e.len;
    const uint64_t b = count::lower_bound(p.doc, lo, hi, first, lane);
    const uint64_t t = last == 0xFFFFFFFFu ? hi : count::lower_bound(p.doc, b, hi, last + 1u, lane);
    if (lane == 0) {
      r_beg[i] = (uint32_t)(b - lo);
      r_end[i] = (uint32_t)(t - lo);
    }
  }
  __syncthreads();
}

// Phase A's question for one entry: is the lane's document `d` among the ids doc[po + rb, po + re)?  Only the lanes
// that `want` search.  A sub-range of up to CONJ_STAGE ids is staged in LDS first - unless no lane of the workgroup
// wants it (the vote is also the barrier behind the last search in the stage) -, a longer one is searched in global
// memory.  Every thread of the workgroup calls, with the same (po, rb, re).
__device__ __forceinline__ bool member(const KParams& p, uint32_t* stage, const uint64_t po, const uint32_t rb, const uint32_t re,
                                       const bool want, const uint32_t d, const int tid) {
  if (re - rb <= CONJ_STAGE) {
    if (!__syncthreads_or(want ? 1 : 0)) return false;
    stage_ids(p.doc, stage, po + rb, po + re, tid);
    __syncthreads();
    const uint32_t len = re - rb;
    return want && find<uint32_t>(stage, 0u, len, d) != len;
  }
  return want && find<uint64_t>(p.doc, po + rb, po + re, d) != po + re;
}

// Compaction: the documents of the live lanes into surv[0 .. n), in lane order, by a ballot prefix; returns n.
__device__ __forceinline__ uint32_t compact(const bool live, const uint32_t d, uint32_t* surv, uint32_t* wave_n) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const unsigned long long lm = __ballot(live);
  if (lane == 0) wave_n[wave] = (uint32_t)__popcll(lm);
  __syncthreads();
  uint32_t base = 0, n_surv = 0;
  for (int w = 0; w < CONJ_WAVES; ++w) {
    if (w < wave) base += wave_n[w];
    n_surv += wave_n[w];
  }
  if (live) surv[base + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull))] = d;
  __syncthreads();
  return n_surv;
}

// Phase B: the exact score of the survivors of an item of query q (entries e0 .. e0 + n - 1, its ranges inside the doc
// ids [first, last] parked already when `once`), one survivor per lane, and their emission into the query's run.
// ALL: a document is emitted iff every one of the query's n_terms terms gave it Some; else iff any posting did.
template <bool ALL>
__device__ __forceinline__ void score_survivors(const KParams& p, uint32_t* r_beg, uint32_t* r_end, const uint32_t* surv, const uint32_t n_surv,
                                                const uint32_t q, const uint32_t e0, const uint32_t n, const uint32_t L, const bool once,
                                                const uint32_t first, const uint32_t last, const uint32_t n_terms,
                                                unsigned long long* run_results) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  if (once && (uint32_t)(wave * WAVE) >= n_surv) return;  // (a wave without a survivor; no barrier below when the ranges are there already)
  const bool has_doc = (uint32_t)tid < n_surv;
  const uint32_t sd = has_doc ? surv[tid] : 0u;
  double score = 0.0;
  bool present = false;
  uint32_t last_term = 0xFFFFFFFFu;
  unsigned long long some = 0ull;
  for (uint32_t i = 0; i < n; ++i) {
    if (!once && i % L == 0) ranges(p, r_beg, r_end, nullptr, e0 + i, min(L, n - i), first, last);  // the next block, in plan order
    const uint32_t slot = once ? i : i % L;
    const uint32_t rb = r_beg[slot], re = r_end[slot];
    if (rb != re && has_doc) {
      const ps_plan_entry e = p.plan[e0 + i];
      const uint64_t pb = e.post_off + rb, pe = e.post_off + re;
      const uint64_t pi = find<uint64_t>(p.doc, pb, pe, sd);
      if (pi != pe) {
        double s = 0.0;
        for (uint32_t x = 0; x < p.F; ++x) {
          const uint32_t w = p.tfl[pi * p.F + x];
          uint32_t tfu = w >> 24, flu = w & TFL_FL_ESC;
          tfl_exact(p, x, pi, tfu, flu);
          if (tfu > 0) s += bm25_tfn(p, x, tfu, flu) * e.idf * p.boost[x] * e.boost;  // bm25.rs:83-86: ((tfn*idf)*boost)*expansion_boost
        }
        if (s > 0.0) {  // Some(score) iff score > 0 (bm25.rs:89-92); max_score_merger (query.rs:150-164)
          score = present ? (last_term == e.qterm ? fmax(score, s) : score + s) : s;
          present = true;
          if (ALL) some |= 1ull << e.qterm;
        }
        last_term = e.qterm;  // visited even when the score was None (query.rs:87)
      }
    }
  }
  const bool emit = has_doc && (ALL ? some == (n_terms >= 64u ? ~0ull : (1ull << n_terms) - 1ull) : present);
  const uint32_t n_emit = (uint32_t)__popcll(__ballot(emit));
  full_emit(p, q, lane, emit, score, sd, EmitFilter{false, 0.0});
  if (lane == 0 && n_emit && run_results != nullptr) atomicAdd(run_results, (unsigned long long)n_emit);
}

}  // namespace conj

__global__ __launch_bounds__(CONJ_NT) void k_conj(const KParams p, const ConjParams a) {
  __shared__ uint32_t r_beg[CONJ_LISTS], r_end[CONJ_LISTS];  // sub-ranges of the current block of entries, relative to their post_off
  __shared__ __align__(16) uint32_t stage[CONJ_STAGE];
  __shared__ uint32_t surv[CONJ_NT];
  __shared__ uint32_t wave_n[CONJ_WAVES];
  const int tid = threadIdx.x;
  const ConjItem it = a.items[blockIdx.x];
  const uint32_t e0 = p.qbeg[it.q], n = p.qbeg[it.q + 1] - e0;
  const uint32_t L = min(max(a.lists, 1u), CONJ_LISTS);
  if (it.count == 0 || it.count > (uint32_t)CONJ_NT) return;  // (the host builds no such item)
  const bool once = n <= L;  // the ranges of the whole query fit: slot of entry e is e - e0, for both phases
  const ps_plan_entry drv = p.plan[it.entry];
  const uint64_t d_at = drv.post_off + it.begin;
  const uint32_t first = p.doc[d_at], last = p.doc[d_at + it.count - 1];
  unsigned long long* ws = p.wstats + (size_t)(blockIdx.x & (WS_SLOTS - 1u)) * WS_WORDS;
  if (PS_WORK_COUNTERS && tid == 0) {
    atomicAdd(&ws[WS_ITEMS], 1ull);
    atomicAdd(&ws[WS_SCANNED], (unsigned long long)it.count);
  }
  if (once) conj::ranges(p, r_beg, r_end, nullptr, e0, n, first, last);

  // ---- phase A: membership ------------------------------------------------------------------------------------------
  // (every branch that holds a barrier depends on the item, the entry and workgroup-wide votes alone)
  const bool mine = (uint32_t)tid < it.count;
  const uint32_t d = mine ? p.doc[d_at + tid] : 0u;
  bool live = mine && doc_alive(p, d);
  bool found = false;
  uint32_t cur = drv.qterm;  // the term whose lists are being searched
  for (uint32_t i = 0; i <= n; ++i) {
    if (!once && i < n && i % L == 0) conj::ranges(p, r_beg, r_end, a.order + e0 + i, 0u, min(L, n - i), first, last);  // the next block, in `order`
    const uint32_t ei = i < n ? a.order[e0 + i] : 0u;
    const uint32_t qt = i < n ? p.plan[ei].qterm : 0xFFFFFFFFu;
    if (qt != cur) {  // a term is through
      if (cur != drv.qterm) live = live && found;
      found = false;
      cur = qt;
      if (!__syncthreads_or(live ? 1 : 0)) return;  // nobody left in the item
    }
    if (i == n) break;
    const bool own_term = qt == drv.qterm;
    if (own_term && ei >= it.entry) continue;  // the item's own list and the later ones of its term
    const uint32_t slot = once ? ei - e0 : i % L;
    const uint32_t rb = r_beg[slot], re = r_end[slot];
    if (rb == re) continue;
    const uint64_t po = p.plan[ei].post_off;
    const bool want = live && !found;
    const bool hit = conj::member(p, stage, po, rb, re, want, d, tid);
    if (own_term) live = live && !hit;  // ownership: an earlier list of the driver term holds the document
    else found = found || hit;
  }

  // ---- compaction, phase B ---------------------------------------------------------------------------------------
  const uint32_t n_surv = conj::compact(live, d, surv, wave_n);
  if (PS_WORK_COUNTERS && tid == 0) atomicAdd(&ws[WS_REACHED], (unsigned long long)n_surv);
  if (n_surv == 0) return;
  conj::score_survivors<true>(p, r_beg, r_end, surv, n_surv, it.q, e0, n, L, once, first, last, a.n_terms[it.q], a.run_results);
}

}  // namespace ps
