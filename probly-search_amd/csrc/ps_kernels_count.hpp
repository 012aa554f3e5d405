// ps_kernels_count.hpp — exact total match counts: Kc k_count_matches, the cardinality of the union of a query's
// doc-sorted lists under the alive bitmap (what `results.len()` of Index::query is, src/query.rs:97-105, without
// scoring, collecting or sorting anything).
//
// A work item is (query, document window): a power-of-two range of doc ids whose bitset lives in dynamic LDS
// (2^19 documents = 64 KiB, two workgroups per CU).  The workgroup
//   * zeroes the bitset,
//   * finds, one wave per list, the postings of every list of the query that fall into the window - two 64-ary
//     searches on the doc-id plane, a probe per lane and a ballot per level (three levels for a list of 2^18),
//   * streams those sub-ranges with 16-byte loads, COUNT_U of them in flight per lane, and sets a bit per posting
//     with an LDS OR whose result nobody reads (ds_or_b32 without return): a document that occurs in several lists -
//     a repeated term, a term and its expansions, terms sharing documents - sets a bit that is set already.
//     Sub-ranges of COUNT_BIG postings and more are streamed by all the waves, shorter ones by one wave each
//     (a prefix query owns hundreds of short lists, a C2 query three long ones),
//   * ANDs every non-empty bitset word with the alive bitmap's word (the window starts at word win << (w_log2 - 5)
//     of the bitmap), popcounts, reduces by shuffles and through LDS, and
//   * adds its sum to totals[q] with ONE global atomic.
// Items are independent: no workgroup waits for another; totals is cleared by a memset on the same stream.
// ZB = true (some fields_boost is 0, none negative): a posting only counts if a field with a positive boost holds the
// term - tf planes of those fields are read beside the doc ids; the common instantiation carries none of that.
// Integer work only, deterministic.  No matrix instruction applies: nothing is multiplied.
#pragma once
#include "ps_kernels_common.hpp"

namespace ps {

constexpr int COUNT_NT = 1024;             // threads per item
constexpr int COUNT_WAVES = COUNT_NT / WAVE;
constexpr int COUNT_U = 4;                 // 16-byte loads per lane in flight
constexpr int COUNT_CHUNK = 64;            // lists whose sub-ranges wait in LDS at a time
constexpr uint32_t COUNT_BIG = 2048;       // postings from which a sub-range is streamed by the whole workgroup
constexpr uint32_t COUNT_MIN_LOG2 = 8, COUNT_MAX_LOG2 = 19, COUNT_AUTO_MIN_LOG2 = 12;

// THE window rule (item builder and launch both take its result from Engine's enqueue_count): log2 of the documents per
// window.  `knob` (PS_COUNT_WINDOW_LOG2) != 0 fixes it.  Otherwise: no wider than the id space, at most 2^19, and
// narrowed - down to 2^12, below which an item's searches outweigh its stream - until the batch offers five items per
// CU (two resident workgroups, two and a half rounds: of 4 / 5 / 6 per CU the one that chooses the best measured width
// for 24, 256 and 1024 queries over 1 M documents - 2^14 / 2^17 / 2^19, EXPERIMENTS.md), so that 24 queries fill the
// chip and 1024 do not zero-fill and popcount more bitsets than they need.
inline uint32_t count_window_log2(const uint64_t n_ids, const uint64_t n_queries, const uint32_t n_cu, const uint32_t knob) {
  if (knob) return knob < COUNT_MIN_LOG2 ? COUNT_MIN_LOG2 : knob > COUNT_MAX_LOG2 ? COUNT_MAX_LOG2 : knob;
  uint32_t l = COUNT_MIN_LOG2;
  while (l < COUNT_MAX_LOG2 && (1ull << l) < n_ids) ++l;
  while (l > COUNT_AUTO_MIN_LOG2 && n_queries * ((n_ids + (1ull << l) - 1) >> l) < 5ull * n_cu) --l;
  return l;
}
inline size_t count_lds_bytes(const uint32_t w_log2) { return (size_t)1 << (w_log2 - 3); }

struct CountList { uint64_t post_off; uint32_t len; uint32_t _pad; };  // a plan entry, as much as counting needs
struct CountItem { uint32_t q, win; };

struct CountParams {
  const uint32_t* doc;       // the doc-id plane
  const uint32_t* tf;        // [F][P] term-frequency planes (ZB only)
  const uint32_t* alive;     // one bit per doc id; null = every document alive
  const CountList* lists;    // [n_plan_entries]
  const uint32_t* qbeg;      // [B + 1]
  const CountItem* items;    // [grid]
  unsigned long long* totals;  // [B], cleared before the launch
  uint64_t P;
  uint32_t n_ids, w_log2, F, pos_fields;  // pos_fields: bit x = fields_boost[x] > 0 (ZB)
};

namespace count {

// First position in [lo, hi) of the ascending plane whose doc id is >= key (hi if none).  All lanes of a wave call
// with the same arguments: every level probes 64 equidistant positions at once.
__device__ __forceinline__ uint64_t lower_bound(const uint32_t* doc, uint64_t lo, uint64_t hi, const uint32_t key, const int lane) {
  while (hi - lo > (uint64_t)WAVE) {
    const uint64_t step = (hi - lo + WAVE - 1) / WAVE, at = lo + (uint64_t)lane * step;
    const uint32_t below = (uint32_t)__popcll(__ballot(at < hi && doc[at] < key));  // the probes are ascending: a prefix of the lanes
    if (below == 0) return lo;
    const uint64_t last = lo + (uint64_t)(below - 1) * step;  // doc[last] < key <= doc[last + step] (if that exists)
    hi = last + step < hi ? last + step : hi;
    lo = last + 1;
  }
  const uint64_t at = lo + (uint64_t)lane;
  return lo + (uint64_t)__popcll(__ballot(at < hi && doc[at] < key));
}

template <bool ZB>
__device__ __forceinline__ void mark(const CountParams& a, uint32_t* bitset, const uint32_t base, const uint32_t d, const uint64_t pos) {
  const uint32_t rel = d - base;
  if (rel >= (1u << a.w_log2) || d >= a.n_ids) return;  // (padding lanes carry ~0; a sorted list has nothing else out here)
  if (ZB) {
    bool holds = false;
    for (uint32_t x = 0; x < a.F; ++x)
      if ((a.pos_fields >> x) & 1u) holds = holds || a.tf[(uint64_t)x * a.P + pos] != 0;
    if (!holds) return;
  }
  atomicOr(&bitset[rel >> 5], 1u << (rel & 31u));
}

// Postings [beg, end) of the plane by `n_thr` threads, this one the r-th: whole 16-byte vectors, the two ragged ends
// element by element (a vector load never leaves the sub-range, so it never leaves the plane).
template <bool ZB>
__device__ __forceinline__ void stream(const CountParams& a, uint32_t* bitset, const uint32_t base, const uint64_t beg, const uint64_t end,
                                       const uint32_t r, const uint32_t n_thr) {
  const uint64_t v0 = beg >> 2, v1 = (end + 3) >> 2;
  const uint4* doc4 = reinterpret_cast<const uint4*>(a.doc);
  for (uint64_t v = v0 + r; v < v1; v += (uint64_t)n_thr * COUNT_U) {
    uint4 x[COUNT_U];
#pragma unroll
    for (int u = 0; u < COUNT_U; ++u) {
      const uint64_t vv = v + (uint64_t)u * n_thr, p = vv << 2;
      x[u] = make_uint4(~0u, ~0u, ~0u, ~0u);
      if (vv >= v1) continue;
      if (p >= beg && p + 4 <= end) {
        x[u] = doc4[vv];
      } else {
        if (p >= beg && p < end) x[u].x = a.doc[p];
        if (p + 1 >= beg && p + 1 < end) x[u].y = a.doc[p + 1];
        if (p + 2 >= beg && p + 2 < end) x[u].z = a.doc[p + 2];
        if (p + 3 >= beg && p + 3 < end) x[u].w = a.doc[p + 3];
      }
    }
#pragma unroll
    for (int u = 0; u < COUNT_U; ++u) {
      const uint64_t p = (v + (uint64_t)u * n_thr) << 2;
      mark<ZB>(a, bitset, base, x[u].x, p);
      mark<ZB>(a, bitset, base, x[u].y, p + 1);
      mark<ZB>(a, bitset, base, x[u].z, p + 2);
      mark<ZB>(a, bitset, base, x[u].w, p + 3);
    }
  }
}

}  // namespace count

template <bool ZB>
__global__ __launch_bounds__(COUNT_NT, ZB ? 4 : 8) void k_count_matches(const CountParams a) {
  extern __shared__ uint4 count_lds[];
  uint32_t* bitset = reinterpret_cast<uint32_t*>(count_lds);
  __shared__ uint64_t r_beg[COUNT_CHUNK], r_end[COUNT_CHUNK];
  __shared__ uint32_t wave_sum[COUNT_WAVES];
  __shared__ uint32_t any;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const CountItem it = a.items[blockIdx.x];
  const uint32_t words = 1u << (a.w_log2 - 5), base = it.win << a.w_log2;
  const uint64_t top = (uint64_t)base + (1ull << a.w_log2);  // first doc id behind the window
  for (uint32_t w = tid; w < words / 4; w += COUNT_NT) count_lds[w] = make_uint4(0u, 0u, 0u, 0u);
  if (tid == 0) any = 0u;
  __syncthreads();  // the bitset and `any` are clear before any wave marks either
  const uint32_t e0 = a.qbeg[it.q], e1 = a.qbeg[it.q + 1];
  for (uint32_t c0 = e0; c0 < e1; c0 += COUNT_CHUNK) {
    const uint32_t n = min((uint32_t)COUNT_CHUNK, e1 - c0);
    for (uint32_t i = wave; i < n; i += COUNT_WAVES) {  // one wave per list
      const CountList l = a.lists[c0 + i];
      const uint64_t lo = l.post_off, hi = l.post_off + l.len;
      const uint64_t b = count::lower_bound(a.doc, lo, hi, base, lane);
      const uint64_t e = top > 0xFFFFFFFFull ? hi : count::lower_bound(a.doc, b, hi, (uint32_t)top, lane);
      if (lane == 0) {
        r_beg[i] = b;
        r_end[i] = e;
        if (e > b) any = 1u;
      }
    }
    __syncthreads();
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t b = r_beg[i], e = r_end[i];
      if (e - b >= COUNT_BIG) count::stream<ZB>(a, bitset, base, b, e, (uint32_t)tid, COUNT_NT);
      else if (e > b && (i % COUNT_WAVES) == (uint32_t)wave) count::stream<ZB>(a, bitset, base, b, e, (uint32_t)lane, WAVE);
    }
    __syncthreads();
  }
  if (!any) return;  // the query has no posting in this window: nothing to popcount
  uint32_t mine = 0;
  const uint32_t word0 = it.win << (a.w_log2 - 5);
  for (uint32_t w = tid; w < words; w += COUNT_NT) {
    uint32_t bits = bitset[w];
    if (bits && a.alive) bits &= a.alive[word0 + w];  // (a set bit is a doc id < n_ids: its word exists)
    mine += (uint32_t)__popc(bits);
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) mine += (uint32_t)__shfl_down((int)mine, d);
  if (lane == 0) wave_sum[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
    for (int w = 0; w < COUNT_WAVES; ++w) sum += wave_sum[w];
    if (sum) atomicAdd(&a.totals[it.q], (unsigned long long)sum);
  }
}

// The slow route's last step: stage 1 of the deep path has counted every query's run (full_cnt); widen the counts into
// the caller's u64 totals before the next slice clears them.
__global__ void k_count_copy(const uint32_t* cnt, unsigned long long* totals, const uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) totals[i] = cnt[i];
}

}  // namespace ps
