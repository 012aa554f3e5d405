// ps_kernels_filter.hpp — query-time document filters (ps_filter, ps_scorer_desc::filter): an allow-list of document
// keys restricts a call's results; scores and order stay the unfiltered query's, bit for bit.
//
// k_filter_build (three small kernels) resolves the keys once, at ps_snapshot_filter_new:
//   k_filter_mark     one thread per key: a binary search in the snapshot's ascending doc id -> key plane, a hit sets the
//                     document's bit in a zeroed bitmap (atomicOr: keys may repeat) laid out like the alive bitmap;
//   k_filter_count    ANDs the alive bitmap in - the result is the ALLOW BITMAP every list-driven stage 1 takes where it
//                     takes the alive bitmap without a filter - and sums the popcounts of each workgroup's 256 words in LDS;
//   k_filter_scan     one workgroup: exclusive prefix sums of the workgroup totals, the grand total (the filter's length);
//   k_filter_scatter  every workgroup scans its words' popcounts again and writes its documents: the filter's sorted,
//                     duplicate-free DOC LIST.
//
// Kf k_filter_score<ALL> is the stage 1 a selective filter drives (BM25, both match modes): instead of streaming every
// posting of the query's lists to keep a handful, the filter's documents are looked up in the lists.  A work item is
// (query, chunk of at most FILTER_CHUNK consecutive documents of the doc list), found from blockIdx alone; one workgroup
// of CONJ_NT threads per item, one filter document per lane:
//   ranges   the chunk spans the doc ids [first, last]: conj::ranges finds every entry's postings inside that span, one
//            wave per entry, CONJ_LISTS entries at a time in LDS.  The chunks of a selective filter are wide, the
//            sub-ranges long but few lanes search them; the chunks of a dense one are narrow and most sub-ranges empty -
//            a workgroup whose sub-ranges are all empty ends at one vote;
//   phase A  membership on doc ids alone (conj::member: staged in LDS up to CONJ_STAGE ids, else global memory).
//            ALL = false: a lane is done at its first hit in any entry, a lane without a hit is dead.  ALL = true: term
//            by term in ascending total length, a lane that misses a term is dead, a lane that found its document skips
//            the term's other lists.  No alive test and no ownership rule: the doc list was compacted from the allow
//            bitmap and holds every document once;
//   compact, phase B   Kj k_conj's (conj::compact, conj::score_survivors): the survivors' exact scores over all entries
//            in plan order with the merger rule; a document is emitted if any posting gave Some (ALL = false) or if
//            every term did (ALL = true: at most CONJ_MAX_TERMS terms).
// It writes the same runs behind full_off / full_cnt as every other stage 1.
#pragma once
#include "ps_kernels_conj.hpp"

namespace ps {

constexpr int FILTER_NT = 256;
constexpr uint32_t FILTER_CHUNK = CONJ_NT;  // filter documents per item (PS_FILTER_CHUNK: 1..CONJ_NT, one per lane)

struct FilterParams {
  const uint32_t* order;     // [n_plan_entries] per query (at qbeg[q]): its entries for phase A (ALL: term by term in ascending total length)
  const uint32_t* n_terms;   // [B] non-empty terms of the query
  const uint32_t* queries;   // [grid / n_chunks] the queries that have a plan entry (ALL: and a posting for every term)
  const uint32_t* docs;      // the filter's doc list, ascending
  unsigned long long* run_results;  // as ConjParams::run_results
  uint32_t n_docs;           // its length
  uint32_t chunk, n_chunks;  // documents per item, items per query = ceil(n_docs / chunk)
  uint32_t lists;            // entries per block of ranges, 1..CONJ_LISTS
};

namespace filter {

// Inclusive prefix sum of one value per thread over the workgroup (s: FILTER_NT words; s[FILTER_NT - 1] is the total
// until the next barrier-separated use).
__device__ __forceinline__ uint32_t block_scan(const uint32_t v, uint32_t* s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int o = 1; o < FILTER_NT; o <<= 1) {
    const uint32_t add = tid >= o ? s[tid - o] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

}  // namespace filter

__global__ __launch_bounds__(FILTER_NT) void k_filter_mark(const uint64_t* keys, const uint64_t n_keys, const uint64_t* doc_keys,
                                                           const uint32_t n_ids, uint32_t* bits) {
  for (uint64_t i = (uint64_t)blockIdx.x * FILTER_NT + threadIdx.x; i < n_keys; i += (uint64_t)gridDim.x * FILTER_NT) {
    const uint64_t key = keys[i];
    uint32_t lo = 0, hi = n_ids;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (doc_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < n_ids && doc_keys[lo] == key) atomicOr(&bits[lo >> 5], 1u << (lo & 31u));
  }
}

// Workgroup b owns the words [b * FILTER_NT, (b + 1) * FILTER_NT) of the bitmap, here and in k_filter_scatter.
__global__ __launch_bounds__(FILTER_NT) void k_filter_count(uint32_t* bits, const uint32_t* alive, const uint32_t n_words, uint32_t* block_tot) {
  __shared__ uint32_t s[FILTER_NT];
  const uint32_t i = blockIdx.x * FILTER_NT + threadIdx.x;
  uint32_t w = 0;
  if (i < n_words) {
    w = bits[i] & alive[i];
    bits[i] = w;
  }
  filter::block_scan((uint32_t)__popc(w), s);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = s[FILTER_NT - 1];
}

// block_tot[0 .. n_blocks) -> its exclusive prefix sums, in place; *total = the sum.
__global__ __launch_bounds__(FILTER_NT) void k_filter_scan(uint32_t* block_tot, const uint32_t n_blocks, uint32_t* total) {
  __shared__ uint32_t s[FILTER_NT];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_blocks; base += FILTER_NT) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_blocks ? block_tot[i] : 0u;
    const uint32_t incl = filter::block_scan(v, s);
    if (i < n_blocks) block_tot[i] = carry + incl - v;
    carry += s[FILTER_NT - 1];
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(FILTER_NT) void k_filter_scatter(const uint32_t* bits, const uint32_t n_words, const uint32_t* block_off, uint32_t* docs) {
  __shared__ uint32_t s[FILTER_NT];
  const uint32_t i = blockIdx.x * FILTER_NT + threadIdx.x;
  uint32_t w = i < n_words ? bits[i] : 0u;
  const uint32_t c = (uint32_t)__popc(w);
  uint32_t o = block_off[blockIdx.x] + filter::block_scan(c, s) - c;
  while (w) {
    docs[o++] = (i << 5) + (uint32_t)(__ffs((int)w) - 1);
    w &= w - 1u;
  }
}

template <bool ALL>
__global__ __launch_bounds__(CONJ_NT) void k_filter_score(const KParams p, const FilterParams a) {
  __shared__ uint32_t r_beg[CONJ_LISTS], r_end[CONJ_LISTS];  // sub-ranges of the current block of entries, relative to their post_off
  __shared__ __align__(16) uint32_t stage[CONJ_STAGE];
  __shared__ uint32_t surv[CONJ_NT];
  __shared__ uint32_t wave_n[CONJ_WAVES];
  const int tid = threadIdx.x;
  const uint32_t q = a.queries[blockIdx.x / a.n_chunks];
  const uint32_t chunk = min(max(a.chunk, 1u), (uint32_t)CONJ_NT);
  const uint32_t begin = (blockIdx.x % a.n_chunks) * chunk;
  const uint32_t e0 = p.qbeg[q], n = p.qbeg[q + 1] - e0;
  const uint32_t L = min(max(a.lists, 1u), CONJ_LISTS);
  if (begin >= a.n_docs || n == 0) return;  // (the host builds no such item)
  const uint32_t count = min(chunk, a.n_docs - begin);
  const uint32_t first = a.docs[begin], last = a.docs[begin + count - 1];
  const bool once = n <= L;  // the ranges of the whole query fit: slot of entry e is e - e0, for both phases
  unsigned long long* ws = p.wstats + (size_t)(blockIdx.x & (WS_SLOTS - 1u)) * WS_WORDS;
  if (PS_WORK_COUNTERS && tid == 0) {
    atomicAdd(&ws[WS_ITEMS], 1ull);
    atomicAdd(&ws[WS_SCANNED], (unsigned long long)count);
  }
  if (once) {
    conj::ranges(p, r_beg, r_end, nullptr, e0, n, first, last);
    bool any = false;
    for (uint32_t i = (uint32_t)tid; i < n; i += CONJ_NT) any = any || r_beg[i] != r_end[i];
    if (!__syncthreads_or(any ? 1 : 0)) return;  // no posting of the query inside the chunk's span
  }

  // ---- phase A: membership ------------------------------------------------------------------------------------------
  // (every branch that holds a barrier depends on the item, the entry and workgroup-wide votes alone)
  const bool mine = (uint32_t)tid < count;
  const uint32_t d = mine ? a.docs[begin + tid] : 0u;
  bool live = mine, found = false;
  uint32_t cur = p.plan[a.order[e0]].qterm;  // ALL: the term whose lists are being searched
  for (uint32_t i = 0; i <= n; ++i) {
    if (!once && i < n && i % L == 0) conj::ranges(p, r_beg, r_end, a.order + e0 + i, 0u, min(L, n - i), first, last);  // the next block, in `order`
    const uint32_t ei = i < n ? a.order[e0 + i] : 0u;
    if (ALL) {
      const uint32_t qt = i < n ? p.plan[ei].qterm : 0xFFFFFFFFu;
      if (qt != cur) {  // a term is through
        live = live && found;
        found = false;
        cur = qt;
        if (!__syncthreads_or(live ? 1 : 0)) return;  // nobody left in the item
      }
    }
    if (i == n) break;
    const uint32_t slot = once ? ei - e0 : i % L;
    const uint32_t rb = r_beg[slot], re = r_end[slot];
    if (rb == re) continue;
    const bool hit = conj::member(p, stage, p.plan[ei].post_off, rb, re, live && !found, d, tid);
    found = found || hit;
  }
  if (!ALL) live = found;

  // ---- compaction, phase B ------------------------------------------------------------------------------------------
  const uint32_t n_surv = conj::compact(live, d, surv, wave_n);
  if (PS_WORK_COUNTERS && tid == 0) atomicAdd(&ws[WS_REACHED], (unsigned long long)n_surv);
  if (n_surv == 0) return;
  conj::score_survivors<ALL>(p, r_beg, r_end, surv, n_surv, q, e0, n, L, once, first, last, a.n_terms[q], a.run_results);
}

}  // namespace ps
