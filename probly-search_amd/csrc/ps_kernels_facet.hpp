// ps_kernels_facet.hpp — facet counts (ps_facet, ps_snapshot_facet_counts_batch*): how the matches of every query of a
// batch spread over the values of a per-document attribute, counts[q][v] = |{d in results(q) : value(d) == v}|, in one
// launch for all values of all queries.
//
// k_facet_build (two small kernels) resolves (key, value) pairs once, at ps_snapshot_facet_new:
//   k_facet_assign  one thread per key: k_filter_mark's binary search in the ascending doc id -> key plane, a hit stores
//                   value + 1 with an atomic max into a zeroed 32-bit build buffer (0 = no value; a key listed more than
//                   once keeps its largest value, whatever the order the threads run in);
//   k_facet_narrow  one thread per document: the build buffer narrowed into the 16-bit VALUE COLUMN the count kernels read
//                   (PS_MAX_FACET_VALUES = 8192 values + "none" fit; 2 bytes per document: the column of 1 M documents
//                   stays in L2), and the alive documents that carry a value counted (a vote per workgroup, one atomic).
//
// Kh k_facet_counts<ZB> is Kc k_count_matches with another reduction.  Same items (query, document window), same gate
// (count_route: FAST / FAST_ZB), same first half: zero the bitset in LDS, find every list's postings inside the window
// (count::lower_bound), stream them (count::stream) and set a bit per posting (count::mark).  Then, instead of a popcount,
//   * the HISTOGRAM - n_values bins, replicated R times, behind the bitset in the same dynamic LDS - is zeroed (an item
//     without a posting in its window has left by then),
//   * the bitset is walked in chunks of 64 documents, 64 chunks per wave and step: every lane reads the two words of its
//     chunk and ANDs them with the emit bitmap's (alive, or alive AND filter: a filter costs nothing more); a ballot of the
//     non-empty chunks drives a loop over those alone - an empty chunk has cost one LDS read, and a sparse query over a
//     wide window is mostly empty chunks.  A non-empty chunk's words are broadcast from its lane, lane l tests bit l, and
//     the lanes whose bit is set read their document's column element - one coalesced load of at most 128 bytes - and add 1
//     to their bin with an LDS atomic whose result nobody reads.  FACET_U chunks are in flight together (their loads are
//     issued before the first add),
//   * the replica is the lane's (lane & (R - 1)), replicas of a bin lie next to each other: the 64 lanes of a chunk whose
//     documents share a value - at n_values = 3 every third document of a dense query - add to R different words in
//     different banks instead of queueing on one.  R is the largest power of two up to 64 for which bitset + R * n_values * 4
//     bytes stay inside FACET_LDS, the 64 KiB that let two workgroups share a CU as k_count_matches' do,
//   * the replicas are summed, a thread per bin (rotated, so that neighbouring threads read different banks), and every
//     non-zero bin of the item is added to counts[q * n_values + v] with one global 64-bit atomic.  counts is cleared by a
//     memset on the same stream.
// Kr k_facet_runs is the last step of the slow route (match-all, a negative boost, k1 / b out of range: count_route's
// COUNT_SLOW): stage 1 of the deep path has written every query's run of matching doc ids; where the count call widens
// full_cnt (k_count_copy), one workgroup per (query, slice of FACET_RUN_SLICE documents of its run) looks the documents
// up in the column and histograms them the same way - replicated LDS bins, one global atomic per non-zero bin.
// Integer work only, deterministic (sums of ones, in any order).  No matrix instruction applies: nothing is multiplied.
#pragma once
#include "ps_kernels_count.hpp"

namespace ps {

constexpr size_t FACET_LDS = 64 * 1024;        // dynamic LDS of an item: bitset + histogram replicas
constexpr int FACET_U = 4;                     // chunks of 64 documents whose column loads are in flight together
constexpr uint32_t FACET_MAX_REPLICAS = 64;
constexpr int FACET_NT = 256;                  // k_facet_build and Kr: threads per workgroup
constexpr uint32_t FACET_RUN_SLICE = 16384;    // Kr: documents of a run per item

// THE window rule of Kh (item builder and launch both take its result from Engine's enqueue_facet_counts):
// count_window_log2's, narrowed further while the bitset and ONE histogram do not fit FACET_LDS together - a 2^19 window
// fills it alone, so Kh never takes one; with 8192 values the window is at most 2^18.  `knob` is clamped by the same cap.
inline uint32_t facet_window_log2(const uint64_t n_ids, const uint64_t n_queries, const uint32_t n_cu, const uint32_t knob, const uint32_t n_values) {
  uint32_t l = count_window_log2(n_ids, n_queries, n_cu, knob);
  while (l > COUNT_MIN_LOG2 && count_lds_bytes(l) + (size_t)n_values * 4 > FACET_LDS) --l;
  return l;
}
// Histogram replicas beside `other` bytes of LDS: the largest power of two up to 64 that fits (1 always does: the window rule).
inline uint32_t facet_replicas(const size_t other, const uint32_t n_values) {
  uint32_t r = FACET_MAX_REPLICAS;
  while (r > 1 && other + (size_t)r * n_values * 4 > FACET_LDS) r >>= 1;
  return r;
}

struct FacetParams {
  const uint16_t* col;         // value + 1 per doc id, 0 = none
  unsigned long long* counts;  // [B][n_values], cleared before the launch
  uint32_t n_values;
  uint32_t r_log2;             // log2 of the histogram replicas
};

namespace facet {

__device__ __forceinline__ void zero(uint32_t* hist, const uint32_t n_words, const int tid, const int n_thr) {
  for (uint32_t i = (uint32_t)tid; i < n_words; i += (uint32_t)n_thr) hist[i] = 0u;
}

// value + 1 of a matched document (0: none) into the lane's replica of its bin.
__device__ __forceinline__ void add(uint32_t* hist, const uint32_t v1, const uint32_t r_log2, const int lane) {
  if (v1) atomicAdd(&hist[((v1 - 1u) << r_log2) + ((uint32_t)lane & ((1u << r_log2) - 1u))], 1u);
}

// The item's histogram into counts[row]: a thread per bin sums its replicas, starting at a replica of its own.
__device__ __forceinline__ void flush(const FacetParams& f, const uint32_t* hist, const uint64_t row, const int tid, const int n_thr) {
  const uint32_t R = 1u << f.r_log2;
  for (uint32_t v = (uint32_t)tid; v < f.n_values; v += (uint32_t)n_thr) {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < R; ++j) sum += hist[(v << f.r_log2) + ((j + v) & (R - 1u))];
    if (sum) atomicAdd(&f.counts[row * f.n_values + v], (unsigned long long)sum);
  }
}

}  // namespace facet

__global__ __launch_bounds__(FACET_NT) void k_facet_assign(const uint64_t* keys, const uint32_t* values, const uint64_t n_keys,
                                                            const uint64_t* doc_keys, const uint32_t n_ids, uint32_t* build) {
  for (uint64_t i = (uint64_t)blockIdx.x * FACET_NT + threadIdx.x; i < n_keys; i += (uint64_t)gridDim.x * FACET_NT) {
    const uint64_t key = keys[i];
    uint32_t lo = 0, hi = n_ids;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (doc_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < n_ids && doc_keys[lo] == key) atomicMax(&build[lo], values[i] + 1u);
  }
}

// n_docs = 32 * the words of the alive bitmap: build, col and alive cover all of it.
__global__ __launch_bounds__(FACET_NT) void k_facet_narrow(const uint32_t* build, const uint32_t* alive, const uint32_t n_docs, uint16_t* col,
                                                            unsigned long long* len) {
  const uint32_t d = blockIdx.x * FACET_NT + threadIdx.x;
  bool counted = false;
  if (d < n_docs) {
    const uint32_t v1 = build[d];
    col[d] = (uint16_t)v1;
    counted = v1 != 0u && ((alive[d >> 5] >> (d & 31u)) & 1u);
  }
  const int n = __syncthreads_count(counted ? 1 : 0);
  if (threadIdx.x == 0 && n) atomicAdd(len, (unsigned long long)n);
}

template <bool ZB>
__global__ __launch_bounds__(COUNT_NT, ZB ? 4 : 8) void k_facet_counts(const CountParams a, const FacetParams f) {
  extern __shared__ uint4 facet_lds[];
  uint32_t* bitset = reinterpret_cast<uint32_t*>(facet_lds);
  __shared__ uint64_t r_beg[COUNT_CHUNK], r_end[COUNT_CHUNK];
  __shared__ uint32_t any;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const CountItem it = a.items[blockIdx.x];
  const uint32_t words = 1u << (a.w_log2 - 5), base = it.win << a.w_log2;
  uint32_t* hist = bitset + words;
  const uint64_t top = (uint64_t)base + (1ull << a.w_log2);  // first doc id behind the window
  for (uint32_t w = tid; w < words / 4; w += COUNT_NT) facet_lds[w] = make_uint4(0u, 0u, 0u, 0u);
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
  if (!any) return;  // the query has no posting in this window: nothing to histogram
  facet::zero(hist, f.n_values << f.r_log2, tid, COUNT_NT);
  __syncthreads();

  // ---- bitset -> histogram ------------------------------------------------------------------------------------------
  const uint32_t chunks = words >> 1, word0 = it.win << (a.w_log2 - 5);
  const uint16_t* col = f.col + base;
  for (uint32_t c0 = (uint32_t)wave * WAVE; c0 < chunks; c0 += COUNT_WAVES * WAVE) {  // (wave-uniform bounds)
    const uint32_t c = c0 + (uint32_t)lane;
    uint32_t lo = 0, hi = 0;
    if (c < chunks) {
      lo = bitset[2 * c];
      hi = bitset[2 * c + 1];
      if (lo && a.alive) lo &= a.alive[word0 + 2 * c];  // (a set bit is a doc id < n_ids: its word exists)
      if (hi && a.alive) hi &= a.alive[word0 + 2 * c + 1];
    }
    unsigned long long todo = __ballot((lo | hi) != 0u);
    while (todo) {
      uint32_t v1[FACET_U];
#pragma unroll
      for (int u = 0; u < FACET_U; ++u) {
        v1[u] = 0u;
        if (!todo) continue;
        const int src = __ffsll(todo) - 1;  // the lane that holds the chunk: wave-uniform
        todo &= todo - 1ull;
        const uint32_t blo = (uint32_t)__shfl((int)lo, src), bhi = (uint32_t)__shfl((int)hi, src);  // (every lane takes part in both)
        if (((lane < 32 ? blo : bhi) >> (lane & 31)) & 1u) v1[u] = col[(size_t)(c0 + (uint32_t)src) * 64u + (uint32_t)lane];
      }
#pragma unroll
      for (int u = 0; u < FACET_U; ++u) facet::add(hist, v1[u], f.r_log2, lane);
    }
  }
  __syncthreads();
  facet::flush(f, hist, it.q, tid, COUNT_NT);
}

struct FacetRunParams {
  const uint32_t* run_doc;   // stage 1's runs of doc ids ...
  const uint64_t* off;       // ... query q's at off[q], cnt[q] long (at most off[q + 1] - off[q])
  const uint32_t* cnt;
  uint32_t n_slices;         // items per query
  uint32_t row0;             // counts row of the slice's first query
  uint32_t n_ids;
};

__global__ __launch_bounds__(FACET_NT) void k_facet_runs(const FacetRunParams a, const FacetParams f) {
  extern __shared__ uint4 facet_lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(facet_lds);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const uint32_t q = blockIdx.x / a.n_slices;
  const uint64_t off = a.off[q], n = min((uint64_t)a.cnt[q], a.off[q + 1] - off);
  const uint64_t beg = (uint64_t)(blockIdx.x % a.n_slices) * FACET_RUN_SLICE, end = min(beg + FACET_RUN_SLICE, n);
  if (beg >= n) return;  // (the grid is sized by the longest run's room)
  facet::zero(hist, f.n_values << f.r_log2, tid, FACET_NT);
  __syncthreads();
  for (uint64_t i = beg + (uint64_t)tid; i < end; i += (uint64_t)FACET_NT * FACET_U) {
    uint32_t v1[FACET_U];
#pragma unroll
    for (int u = 0; u < FACET_U; ++u) {
      const uint64_t at = i + (uint64_t)u * FACET_NT;
      v1[u] = 0u;
      if (at >= end) continue;
      const uint32_t d = a.run_doc[off + at];
      if (d < a.n_ids) v1[u] = f.col[d];
    }
#pragma unroll
    for (int u = 0; u < FACET_U; ++u) facet::add(hist, v1[u], f.r_log2, lane);
  }
  __syncthreads();
  facet::flush(f, hist, (uint64_t)a.row0 + q, tid, FACET_NT);
}

}  // namespace ps
