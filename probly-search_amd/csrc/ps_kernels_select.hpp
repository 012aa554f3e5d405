// ps_kernels_select.hpp — deep top-k (64 < K <= PS_MAX_DEEP_TOPK): k_deep_offsets + K4s k_deep_select, and result
// pages (ranks [skip, skip + K) for skip > 0): K4w k_deep_window, a two-sided form of the same select; and, at the end,
// Kt k_deep_threshold, which runs INSIDE stage 1 and lets its second launch emit only what can reach rank skip + K.
//
// Stage 1 is full-result mode's (k_score<.., FULL> / k_z21<true>): every query's run of (doc, score) behind
// full_off / full_cnt.  k_deep_select then picks the first K of the run's canonical order (score desc, doc asc)
// without sorting the run: one workgroup of 1024 threads per query does an MSD radix SELECT over the key
//   { score bits 62..0 (scores are >= +0.0 here, ps_sort.hip: the bit pattern orders like the number) , ~doc }
// - 95 bits, unique inside a run (a document occurs once), so there are exactly min(K, n) winners - in eight levels
// of 12 / 12 / 12 / 12 / 12 / 3+9 / 12 / 11 bits.  A level is a 4096-bin LDS histogram of the elements that still
// share the pivot prefix, a suffix scan that finds the pivot bin, and ONE streaming pass that
//   * appends what lies above the pivot bin to the winners (LDS, at most K),
//   * compacts the pivot bin - into the LDS candidate buffer when the histogram says it fits (DEEP_CAND elements),
//     else into the other one of the two global buffers (the run itself / the sort scratch; never in place), and
//     only when that at least halves the source: the top level is mostly exponent, its pivot bin is most of the run,
//     and a run of equal scores has ONE bin on every score level - then the source stays and the prefix filters -,
//   * histograms the next level of what it kept.
// Once the candidates sit in LDS they stay where they are and only the prefix narrows.  It ends when the pivot bin
// holds exactly what is still needed; the winners are sorted in LDS (bitonic) and written as k_merge writes its rows.
// Histogram adds are wave-aggregated for the first DEEP_PEEL distinct digits of a wave-wide load (the commonest
// exponent digit, equal scores: 64 lanes on one bin) and plain LDS atomics for the rest (mantissa digits hardly collide).
// No matrix instruction applies: the kernel moves and counts keys, it computes nothing.
#pragma once
#include "ps_kernels_common.hpp"

namespace ps {

constexpr int DEEP_NT = 1024;            // threads per query
constexpr int DEEP_WAVES = DEEP_NT / WAVE;
constexpr int DEEP_BINS = 4096;          // 12-bit digits
constexpr int DEEP_LEVELS = 8;
constexpr int DEEP_CAND = 8192;          // LDS candidate buffer, elements
constexpr int DEEP_MAX_K = PS_MAX_DEEP_TOPK;
constexpr int DEEP_U = 4;                // 8-byte loads per lane in flight
constexpr int DEEP_PEEL = 1;             // distinct digits of a wave-wide load added once per wave (4 measured slower: the rounds cost more issue slots than the conflicts they save)
// LDS: histogram 16 KiB | candidate scores 64 KiB | candidate docs 32 KiB | winner scores 8 KiB | winner docs 4 KiB | control
constexpr size_t DEEP_LDS = (size_t)DEEP_BINS * 4 + (size_t)DEEP_CAND * 12 + (size_t)DEEP_MAX_K * 12 + 128;
static_assert(DEEP_BINS % DEEP_NT == 0 && DEEP_LDS <= 160 * 1024, "k_deep_select's LDS plan");

struct DeepParams {
  uint32_t* run_doc;        // stage 1's runs (full_doc / full_score); the second compaction of a long run reuses them
  uint64_t* run_score;
  uint32_t* tmp_doc;        // the sort path's scratch (d_sort_doc / d_sort_score), same offsets
  uint64_t* tmp_score;
  const uint64_t* off;      // [n + 1] run q is [off[q], off[q + 1]) at most
  const uint32_t* cnt;      // [n] what stage 1 emitted
  const uint64_t* keys;
  uint64_t* out_keys;       // the caller's block: row0 + q is this launch's q-th query
  double* out_scores;
  uint32_t* out_counts;
  uint32_t K, row0;
  unsigned long long* run_results;  // ps_work_counters::run_results: every query adds the length of the run it selects from
};

// Run offsets of a deep batch on the device: off[q] = sum over earlier queries of min(n_docs, sum of list lengths) -
// the bound the host sized the buffers with -, cnt[q] = 0.  One workgroup.
__global__ __launch_bounds__(DEEP_NT) void k_deep_offsets(const ps_plan_entry* plan, const uint32_t* qbeg, uint32_t B,
                                                          uint32_t n_docs, uint64_t* off, uint32_t* cnt) {
  __shared__ uint64_t wave_tot[DEEP_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const uint32_t per = (B + DEEP_NT - 1) / DEEP_NT;
  const uint32_t q0 = min(B, threadIdx.x * per), q1 = min(B, q0 + per);
  auto cap_of = [&](uint32_t q) {
    uint64_t sum = 0;
    for (uint32_t e = qbeg[q]; e < qbeg[q + 1]; ++e) sum += plan[e].len;
    return sum < n_docs ? sum : (uint64_t)n_docs;
  };
  uint64_t mine = 0;
  for (uint32_t q = q0; q < q1; ++q) mine += cap_of(q);
  uint64_t incl = mine;
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint64_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == WAVE - 1) wave_tot[wave] = incl;
  __syncthreads();
  uint64_t at = incl - mine;
  for (int w = 0; w < wave; ++w) at += wave_tot[w];
  for (uint32_t q = q0; q < q1; ++q) {
    off[q] = at;
    cnt[q] = 0;
    at += cap_of(q);
  }
  if (threadIdx.x == DEEP_NT - 1) off[B] = at;  // (the last thread's range ends at B whatever `per` is)
}

namespace deep {

struct Level { uint32_t s_shift, s_bits, d_shift, d_bits; };  // a digit: s_bits of the score above d_bits of ~doc
__device__ __forceinline__ Level level_of(const int l) {
  if (l < 5) return Level{(uint32_t)(51 - 12 * l), 12u, 0u, 0u};
  if (l == 5) return Level{0u, 3u, 23u, 9u};
  return l == 6 ? Level{0u, 0u, 11u, 12u} : Level{0u, 0u, 0u, 11u};
}
__device__ __forceinline__ uint32_t digit_of(const Level g, const uint64_t s, const uint32_t nd) {
  return ((uint32_t)(s >> g.s_shift) & ((1u << g.s_bits) - 1u)) << g.d_bits | ((nd >> g.d_shift) & ((1u << g.d_bits) - 1u));
}
struct Prefix {  // the pivot digits so far: an element is still a candidate while (key & mask) == value
  uint64_t s_mask = 0, s_val = 0;
  uint32_t d_mask = 0, d_val = 0;
  __device__ __forceinline__ void push(const Level g, const uint32_t pivot) {
    s_mask |= (uint64_t)((1u << g.s_bits) - 1u) << g.s_shift;
    s_val |= (uint64_t)(pivot >> g.d_bits) << g.s_shift;
    d_mask |= ((1u << g.d_bits) - 1u) << g.d_shift;
    d_val |= (pivot & ((1u << g.d_bits) - 1u)) << g.d_shift;
  }
};

struct Ctl {  // LDS control words (pivot2 .. pop2: the second target of k_deep_window's two-sided descent)
  uint32_t n_win, n_dst, pivot, above, pop, pivot2, above2, pop2;
  uint32_t wave_tot[DEEP_WAVES];
};

// hist[digit]++ for the lanes where `on`; all lanes of the wave call.
__device__ __forceinline__ void hist_add(uint32_t* hist, const int lane, const bool on, const uint32_t digit) {
  unsigned long long todo = __ballot(on);
#pragma unroll
  for (int r = 0; r < DEEP_PEEL; ++r) {
    if (!todo) break;
    const int lead = __ffsll(todo) - 1;
    const uint32_t v = readlane_u32(digit, lead);
    const unsigned long long same = __ballot(on && digit == v) & todo;
    if (lane == lead) atomicAdd(&hist[v], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&hist[digit], 1u);
}
// One reservation per wave: the slot of this lane's element behind *counter (lanes where `on`); all lanes call.
__device__ __forceinline__ uint32_t wave_slot(uint32_t* counter, const int lane, const bool on) {
  const unsigned long long m = __ballot(on);
  if (!m) return 0u;
  const int lead = __ffsll(m) - 1;
  uint32_t base = 0;
  if (lane == lead) base = atomicAdd(counter, (uint32_t)__popcll(m));
  return readlane_u32(base, lead) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// One pass over src[0, m): of the elements that match `pre`,
//   sel_lvl >= 0: digit > pivot -> winners, digit < pivot -> dropped, digit == pivot -> kept (take_pivot: winners too);
//   kept elements go to dst (when there is one; dst_cap elements) and into the histogram of hist_lvl (when >= 0).
// k_deep_window's two additions: digits are taken XOR `flip` (0, or DEEP_BINS - 1: the order mirrored, so that the
// same descent selects from the bottom), and a digit above `top` is dropped instead of won (the window's upper side).
// Every thread of the workgroup calls with the same arguments.
__device__ __forceinline__ void select_pass(const uint64_t* src_s, const uint32_t* src_d, const uint64_t m, const Prefix pre,
                                            const int sel_lvl, const uint32_t pivot, const bool take_pivot, const int hist_lvl,
                                            uint64_t* dst_s, uint32_t* dst_d, const uint32_t dst_cap, uint32_t* hist,
                                            uint64_t* win_s, uint32_t* win_d, Ctl* ctl, const uint32_t flip = 0u,
                                            const uint32_t top = ~0u) {
  const int lane = threadIdx.x & (WAVE - 1);
  const Level gs = level_of(sel_lvl < 0 ? 0 : sel_lvl), gh = level_of(hist_lvl < 0 ? 0 : hist_lvl);
  // the doc id is only fetched by a pass that looks at it or moves it
  const bool want_doc = sel_lvl >= 0 || dst_s != nullptr || hist_lvl >= 5 || pre.d_mask != 0;
  for (uint64_t base = 0; base < m; base += (uint64_t)DEEP_NT * DEEP_U) {
    uint64_t s[DEEP_U];
    uint32_t nd[DEEP_U];
#pragma unroll
    for (int u = 0; u < DEEP_U; ++u) {
      const uint64_t i = base + (uint64_t)u * DEEP_NT + threadIdx.x;
      s[u] = i < m ? src_s[i] : 0ull;
      nd[u] = (want_doc && i < m) ? ~src_d[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < DEEP_U; ++u) {
      const uint64_t i = base + (uint64_t)u * DEEP_NT + threadIdx.x;
      const bool act = i < m && (s[u] & pre.s_mask) == pre.s_val && (nd[u] & pre.d_mask) == pre.d_val;
      bool win = false, keep = act;
      if (sel_lvl >= 0) {
        const uint32_t dg = digit_of(gs, s[u], nd[u]) ^ flip;
        win = act && (dg > pivot || (take_pivot && dg == pivot)) && dg <= top;
        keep = act && dg == pivot && !take_pivot;
        const uint32_t w = wave_slot(&ctl->n_win, lane, win);
        if (win && w < (uint32_t)DEEP_MAX_K) { win_s[w] = s[u]; win_d[w] = ~nd[u]; }
      }
      if (dst_s != nullptr) {
        const uint32_t o = wave_slot(&ctl->n_dst, lane, keep);
        if (keep && o < dst_cap) { dst_s[o] = s[u]; dst_d[o] = ~nd[u]; }
      }
      if (hist_lvl >= 0) hist_add(hist, lane, keep, digit_of(gh, s[u], nd[u]) ^ flip);
    }
  }
}

// The pivot bin of the histogram for `need` elements from the top: ctl->pivot, ->above (elements in higher bins),
// ->pop (elements in it) - or ->pivot2, ->above2, ->pop2 for `second`.  need >= 1 and the histogram holds at least
// `need`.  Ends with a barrier.  NT: threads of the workgroup (k_deep_threshold's is narrower).
template <int NT = DEEP_NT>
__device__ __forceinline__ void find_pivot(const uint32_t* hist, const uint32_t need, Ctl* ctl, const bool second = false) {
  constexpr int PER = DEEP_BINS / NT;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const int top = DEEP_BINS - 1 - (int)threadIdx.x * PER;  // this thread's bins: top, top - 1, ... (descending digits)
  uint32_t h[PER], mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) { h[j] = hist[top - j]; mine += h[j]; }
  uint32_t incl = mine;
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == WAVE - 1) ctl->wave_tot[wave] = incl;
  __syncthreads();
  uint32_t above = incl - mine;
  for (int w = 0; w < wave; ++w) above += ctl->wave_tot[w];
  if (above < need && need - above <= mine) {  // the crossing lies in this thread's bins
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (above < need && need - above <= h[j]) {
        if (second) { ctl->pivot2 = (uint32_t)(top - j); ctl->above2 = above; ctl->pop2 = h[j]; }
        else { ctl->pivot = (uint32_t)(top - j); ctl->above = above; ctl->pop = h[j]; }
      }
      above += h[j];
    }
  }
  __syncthreads();
}

template <int NT = DEEP_NT>
__device__ __forceinline__ void clear_hist(uint32_t* hist) {
  for (int b = threadIdx.x; b < DEEP_BINS; b += NT) hist[b] = 0u;
}

// The end of both select kernels: bitonic sort of the n_win winners (LDS), padded to a power of two with keys below
// every real one, then row row0 + q of the caller's block: winners [first, first + n_out), padding, the count.
__device__ __forceinline__ void sort_and_write(const DeepParams& a, const uint32_t q, uint64_t* win_s, uint32_t* win_d,
                                               const uint32_t n_win, const uint32_t first, const uint32_t n_out) {
  const uint32_t K = a.K;
  uint32_t P = 1;
  while (P < n_win) P <<= 1;
  for (uint32_t i = n_win + threadIdx.x; i < P; i += DEEP_NT) { win_s[i] = 0ull; win_d[i] = 0xFFFFFFFFu; }
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const uint32_t i = threadIdx.x, x = i ^ j;
      if (i < P && x > i) {
        const uint64_t si = win_s[i], sx = win_s[x];
        const uint32_t di = win_d[i], dx = win_d[x];
        const bool i_first = si > sx || (si == sx && di < dx);  // canonical order: score desc, doc asc
        if (((i & k) == 0) != i_first) { win_s[i] = sx; win_d[i] = dx; win_s[x] = si; win_d[x] = di; }
      }
      __syncthreads();
    }
  }
  const uint64_t row = (uint64_t)(a.row0 + q) * K;
  for (uint32_t i = threadIdx.x; i < K; i += DEEP_NT) {
    const bool ok = i < n_out;
    a.out_keys[row + i] = ok ? a.keys[win_d[first + i]] : ~0ull;
    a.out_scores[row + i] = ok ? __longlong_as_double((long long)win_s[first + i]) : 0.0;
  }
  if (threadIdx.x == 0) a.out_counts[a.row0 + q] = n_out;
}

}  // namespace deep

// K4s: the first K of every run's canonical order into the caller's [B*K keys | B*K scores | B counts] block.
__global__ __launch_bounds__(DEEP_NT) void k_deep_select(const DeepParams a) {
  using namespace deep;
  extern __shared__ __align__(16) unsigned char deep_lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(deep_lds);
  uint64_t* cand_s = reinterpret_cast<uint64_t*>(deep_lds + (size_t)DEEP_BINS * 4);
  uint64_t* win_s = cand_s + DEEP_CAND;
  uint32_t* cand_d = reinterpret_cast<uint32_t*>(win_s + DEEP_MAX_K);
  uint32_t* win_d = cand_d + DEEP_CAND;
  Ctl* ctl = reinterpret_cast<Ctl*>(win_d + DEEP_MAX_K);

  const uint32_t q = blockIdx.x, K = a.K;
  const uint64_t off = a.off[q];
  const uint64_t n = min((uint64_t)a.cnt[q], a.off[q + 1] - off);
  uint32_t n_out = (uint32_t)min((uint64_t)K, n);
  if (threadIdx.x == 0) { ctl->n_win = 0; ctl->n_dst = 0; atomicAdd(a.run_results, (unsigned long long)n); }
  clear_hist(hist);
  __syncthreads();

  if (n <= K) {  // the whole run: only the sort
    for (uint32_t i = threadIdx.x; i < (uint32_t)n; i += DEEP_NT) { win_s[i] = a.run_score[off + i]; win_d[i] = a.run_doc[off + i]; }
  } else {
    Prefix pre;
    select_pass(a.run_score + off, a.run_doc + off, n, pre, -1, 0u, false, 0, nullptr, nullptr, 0u, hist, win_s, win_d, ctl);
    __syncthreads();
    // where the candidates are: a global buffer (the run, then alternating with the scratch) or the LDS buffer
    const uint64_t* src_s = a.run_score + off;
    const uint32_t* src_d = a.run_doc + off;
    uint64_t m = n;
    bool in_lds = false, in_tmp = false;
    uint32_t need = K;
    for (int lvl = 0; lvl < DEEP_LEVELS; ++lvl) {
      find_pivot(hist, need, ctl);
      const uint32_t pivot = ctl->pivot, pop = ctl->pop;
      need -= ctl->above;
      // (keys are unique, so the last level's bins hold one element each and it always ends here)
      const bool last = pop == need || lvl == DEEP_LEVELS - 1;
      const bool to_lds = !last && !in_lds && pop <= (uint32_t)DEEP_CAND;
      const bool to_glb = !last && !in_lds && !to_lds && (uint64_t)pop <= m / 2;
      __syncthreads();  // every thread has read ctl and the histogram
      clear_hist(hist);
      if (threadIdx.x == 0) ctl->n_dst = 0;
      __syncthreads();
      const int hist_lvl = last ? -1 : lvl + 1;
      if (in_lds) {
        select_pass(cand_s, cand_d, m, pre, lvl, pivot, last, hist_lvl, nullptr, nullptr, 0u, hist, win_s, win_d, ctl);
      } else {
        uint64_t* const glb_s = (in_tmp ? a.run_score : a.tmp_score) + off;  // the global buffer the source is not in
        uint32_t* const glb_d = (in_tmp ? a.run_doc : a.tmp_doc) + off;
        select_pass(src_s, src_d, m, pre, lvl, pivot, last, hist_lvl, to_lds ? cand_s : to_glb ? glb_s : nullptr,
                    to_lds ? cand_d : to_glb ? glb_d : nullptr, pop, hist, win_s, win_d, ctl);
        if (to_glb) { src_s = glb_s; src_d = glb_d; in_tmp = !in_tmp; }
        if (to_lds || to_glb) m = pop;
        in_lds = to_lds;
      }
      pre.push(level_of(lvl), pivot);
      __threadfence_block();
      __syncthreads();  // (a global destination is read back by this workgroup only)
      if (last) break;
    }
  }
  __syncthreads();
  if (n > K) n_out = min(K, ctl->n_win);  // (== K: the winners are exactly the K largest keys)
  sort_and_write(a, q, win_s, win_d, n_out, 0u, n_out);
}

// K4w: ranks [skip, skip + K) of every run's canonical order (a result page) into the same block; skip > 0.
// With lo = skip and hi = min(n, skip + K):
//   lo >= n            padding only;
//   n <= DEEP_MAX_K    the whole run is sorted in LDS and [lo, hi) of it written;
//   hi <= DEEP_MAX_K   k_deep_select's one-sided descent for the top hi, then [lo, hi) of the sorted winners;
//   hi >  DEEP_MAX_K   a two-sided descent: what lies above the window is unbounded and is never collected.
// The two-sided descent is ONE loop over the levels in three roles.  TRUNK: both targets (rank lo and rank hi - 1)
// are looked up in the same histogram; while they fall into the same bin the pass keeps that bin only (no winners)
// and compacts it by k_deep_select's rules.  PARTING level: the bins strictly between the two pivot bins are winners
// outright (their ranks lie inside the window), a boundary bin that lies wholly inside is too; nothing is compacted
// here - both tails start from where the trunk left the candidates (a trunk that reached LDS serves both from LDS).
// TAILS: the lower boundary bin gives its highest hi - above_hi elements - a one-sided descent as in k_deep_select,
// whose first histogram the parting pass made -, then the upper boundary bin gives its lowest above_lo + pop_lo - lo:
// the same descent over mirrored digits (flip), after one counting pass of its own.  While the upper tail waits, the
// lower one must not compact into the global buffer the trunk's candidates are in (it may use the other one, once).
// Passes over a run of distinct scores: k_deep_select's own when the targets part after the candidates reached LDS
// (parting, tails and the counting pass then work in LDS); when they part while the candidates are still a global
// buffer, up to three more over that buffer - the parting pass (wins and counts, does not compact), the lower tail's
// first pass and the upper tail's counting pass - before each tail has compacted its bin.  DESIGN.md section 3.
__global__ __launch_bounds__(DEEP_NT) void k_deep_window(const DeepParams a, const uint32_t skip) {
  using namespace deep;
  extern __shared__ __align__(16) unsigned char deep_lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(deep_lds);
  uint64_t* cand_s = reinterpret_cast<uint64_t*>(deep_lds + (size_t)DEEP_BINS * 4);
  uint64_t* win_s = cand_s + DEEP_CAND;
  uint32_t* cand_d = reinterpret_cast<uint32_t*>(win_s + DEEP_MAX_K);
  uint32_t* win_d = cand_d + DEEP_CAND;
  Ctl* ctl = reinterpret_cast<Ctl*>(win_d + DEEP_MAX_K);

  const uint32_t q = blockIdx.x, K = a.K;
  const uint64_t off = a.off[q];
  const uint64_t n = min((uint64_t)a.cnt[q], a.off[q + 1] - off);
  const uint64_t hi = min(n, (uint64_t)skip + K);
  const uint32_t n_out = skip < n ? (uint32_t)(hi - skip) : 0u;
  uint32_t n_win = 0, first = 0;  // winners to sort; where the window begins among them
  if (threadIdx.x == 0) { ctl->n_win = 0; ctl->n_dst = 0; atomicAdd(a.run_results, (unsigned long long)n); }
  clear_hist(hist);
  __syncthreads();

  if (n_out == 0) {  // the page lies behind the run
  } else if (n <= (uint64_t)DEEP_MAX_K) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)n; i += DEEP_NT) { win_s[i] = a.run_score[off + i]; win_d[i] = a.run_doc[off + i]; }
    n_win = (uint32_t)n;
    first = skip;
  } else {
    const bool two_sided = hi > (uint64_t)DEEP_MAX_K;
    const uint64_t* src_s = a.run_score + off;
    const uint32_t* src_d = a.run_doc + off;
    uint64_t m = n;
    bool in_lds = false, in_tmp = false;
    Prefix pre;
    bool trunk = two_sided;
    uint32_t t_lo = skip + 1u, t_hi = (uint32_t)hi;  // the targets, counted from the top of the candidates (a tail has t_hi only)
    uint32_t flip = 0u;
    // the upper tail while the lower one runs: its prefix, level, count, and the trunk's candidates
    bool up_waits = false, up_in_lds = false, up_in_tmp = false;
    Prefix up_pre;
    int up_lvl = 0;
    uint32_t up_need = 0u;
    const uint64_t* up_src_s = nullptr;
    const uint32_t* up_src_d = nullptr;
    uint64_t up_m = 0;
    bool count_first = true;  // the histogram of `lvl` is still to be made
    for (int lvl = 0;;) {
      if (count_first) {
        if (in_lds) select_pass(cand_s, cand_d, m, pre, -1, 0u, false, lvl, nullptr, nullptr, 0u, hist, win_s, win_d, ctl, flip);
        else select_pass(src_s, src_d, m, pre, -1, 0u, false, lvl, nullptr, nullptr, 0u, hist, win_s, win_d, ctl, flip);
        __syncthreads();
        count_first = false;
      }
      uint32_t pivot, pop, top = ~0u, up_pivot = 0u;
      bool last, part = false;
      if (trunk) {
        find_pivot(hist, t_lo, ctl);
        find_pivot(hist, t_hi, ctl, true);
        const uint32_t p_lo = ctl->pivot, above_lo = ctl->above, pop_lo = ctl->pop;
        const uint32_t p_hi = ctl->pivot2, above_hi = ctl->above2, pop_hi = ctl->pop2;
        if (p_lo == p_hi) {  // one bin holds the window: keep it, win nothing - unless it IS the window
          pivot = p_lo; pop = pop_lo; top = p_lo;
          t_lo -= above_lo;
          t_hi -= above_lo;
          last = (t_lo == 1u && t_hi == pop_lo) || lvl == DEEP_LEVELS - 1;
        } else {  // the targets part (p_lo > p_hi)
          part = true;
          const uint32_t c_lo = above_lo + pop_lo - (t_lo - 1u), c_hi = t_hi - above_hi;  // what the boundary bins contribute
          up_waits = c_lo != pop_lo;
          up_pivot = p_lo; up_need = c_lo;
          pivot = p_hi; pop = pop_hi; top = up_waits ? p_lo - 1u : p_lo;
          t_hi = c_hi;
          last = c_hi == pop_hi;
        }
      } else {
        find_pivot(hist, t_hi, ctl);
        pivot = ctl->pivot; pop = ctl->pop;
        t_hi -= ctl->above;
        last = pop == t_hi || lvl == DEEP_LEVELS - 1;
      }
      uint64_t* const glb_s = (in_tmp ? a.run_score : a.tmp_score) + off;  // the global buffer the source is not in
      uint32_t* const glb_d = (in_tmp ? a.run_doc : a.tmp_doc) + off;
      const bool may_move = !last && !part && !in_lds;
      const bool to_lds = may_move && pop <= (uint32_t)DEEP_CAND;
      const bool to_glb = may_move && !to_lds && (uint64_t)pop <= m / 2 && !(up_waits && glb_s == up_src_s);
      __syncthreads();  // every thread has read ctl and the histogram
      clear_hist(hist);
      if (threadIdx.x == 0) ctl->n_dst = 0;
      __syncthreads();
      const int hist_lvl = last ? -1 : lvl + 1;
      if (in_lds) {
        select_pass(cand_s, cand_d, m, pre, lvl, pivot, last, hist_lvl, nullptr, nullptr, 0u, hist, win_s, win_d, ctl, flip, top);
      } else {
        select_pass(src_s, src_d, m, pre, lvl, pivot, last, hist_lvl, to_lds ? cand_s : to_glb ? glb_s : nullptr,
                    to_lds ? cand_d : to_glb ? glb_d : nullptr, pop, hist, win_s, win_d, ctl, flip, top);
      }
      if (part) {  // the trunk ends: its candidates stay where they are for the upper tail
        up_pre = pre;
        up_pre.push(level_of(lvl), up_pivot);
        up_lvl = lvl + 1;
        up_src_s = src_s; up_src_d = src_d; up_m = m; up_in_lds = in_lds; up_in_tmp = in_tmp;
        trunk = false;
      }
      if (to_glb) { src_s = glb_s; src_d = glb_d; in_tmp = !in_tmp; }
      if (to_lds || to_glb) m = pop;
      if (to_lds) in_lds = true;
      pre.push(level_of(lvl), pivot ^ flip);
      ++lvl;
      __threadfence_block();
      __syncthreads();  // (a global destination is read back by this workgroup only)
      if (last) {  // this descent is complete
        if (!up_waits) break;
        up_waits = false;
        pre = up_pre; lvl = up_lvl; t_hi = up_need;
        src_s = up_src_s; src_d = up_src_d; m = up_m; in_lds = up_in_lds; in_tmp = up_in_tmp;
        flip = (uint32_t)DEEP_BINS - 1u;
        count_first = true;
      }
    }
    n_win = min((uint32_t)DEEP_MAX_K, ctl->n_win);  // (== hi one-sided, == hi - lo two-sided: keys are unique)
    first = two_sided ? 0u : skip;
  }
  __syncthreads();
  sort_and_write(a, q, win_s, win_d, n_win, first, n_out);
}

// Kt: k_deep_threshold - between the two launches of a thresholded stage 1 (ps_engine.hip: score_into_runs).  The run
// holds what the first launch emitted: every match among the documents of the first runs.  thr[q] = the bit pattern of
// the hi-th largest SCORE of that run (hi = skip + top_k), +0.0 when the run holds fewer than hi: a lower bound of the
// query's final hi-th best score, so the second launch may drop every document that scores strictly below it.
// One workgroup per query, an MSD counting descent as in K4s but over the 63 score bits alone - scores repeat, so the
// descent always takes its six levels (12 / 12 / 12 / 12 / 12 / 3 bits) and ends on one value, not on one element - and
// it only counts: no winners, no sort, no doc ids, no global scratch.  The first pass histograms level 0 of the whole
// run; every later level is one pass over the candidates - the run, filtered by the pivot prefix, until the pivot bin
// fits the LDS candidate buffer (that pass compacts it: scores only), the LDS buffer from then on.  A bin that never
// fits (a long block of equal scores) is re-filtered in place on every level, which is K4s's tie rule.
// THR_NT = 512: the run is a sample (about 1/16 of the query's matches), a pass is a few loads per lane, and what is
// left - six pivot searches over 4096 bins and the barriers around them - is cheaper with 8 waves than with 16.
// LDS: histogram 16 KiB | candidate scores 56 KiB | control: 73 856 B, so two workgroups share a CU's 160 KiB.
constexpr int THR_NT = 512;
constexpr int THR_LEVELS = 6;
constexpr int THR_CAND = 7168;
constexpr size_t THR_LDS = (size_t)DEEP_BINS * 4 + (size_t)THR_CAND * 8 + 128;
static_assert(DEEP_BINS % THR_NT == 0 && THR_NT / WAVE <= DEEP_WAVES && sizeof(deep::Ctl) <= 128 && 2 * THR_LDS <= 160 * 1024,
              "k_deep_threshold's LDS plan");

namespace deep {
// One pass over src[0, m) (the run, or the LDS candidates): the scores that match `pre` go into the histogram of
// hist_lvl and, when there is one, to dst (dst_cap elements).  Every thread of the workgroup calls with the same arguments.
__device__ __forceinline__ void threshold_pass(const uint64_t* src, const uint64_t m, const Prefix pre, const int hist_lvl,
                                               uint64_t* dst, const uint32_t dst_cap, uint32_t* hist, Ctl* ctl) {
  const int lane = threadIdx.x & (WAVE - 1);
  const Level gh = level_of(hist_lvl);
  for (uint64_t base = 0; base < m; base += (uint64_t)THR_NT * DEEP_U) {
    uint64_t s[DEEP_U];
#pragma unroll
    for (int u = 0; u < DEEP_U; ++u) {
      const uint64_t i = base + (uint64_t)u * THR_NT + threadIdx.x;
      s[u] = i < m ? src[i] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < DEEP_U; ++u) {
      const uint64_t i = base + (uint64_t)u * THR_NT + threadIdx.x;
      const bool act = i < m && (s[u] & pre.s_mask) == pre.s_val;
      if (dst != nullptr) {
        const uint32_t o = wave_slot(&ctl->n_dst, lane, act);
        if (act && o < dst_cap) dst[o] = s[u];
      }
      hist_add(hist, lane, act, digit_of(gh, s[u], 0u));
    }
  }
}
}  // namespace deep

__global__ __launch_bounds__(THR_NT) void k_deep_threshold(const uint64_t* run_score, const uint64_t* off, const uint32_t* cnt,
                                                           const uint32_t hi, unsigned long long* thr) {
  using namespace deep;
  extern __shared__ __align__(16) unsigned char deep_lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(deep_lds);
  uint64_t* cand = reinterpret_cast<uint64_t*>(deep_lds + (size_t)DEEP_BINS * 4);
  Ctl* ctl = reinterpret_cast<Ctl*>(cand + THR_CAND);

  const uint32_t q = blockIdx.x;
  const uint64_t o = off[q];
  const uint64_t n = min((uint64_t)cnt[q], off[q + 1] - o);
  if (n < (uint64_t)hi) {  // the sample cannot bound the hi-th best: the second launch emits everything
    if (threadIdx.x == 0) thr[q] = 0ull;
    return;
  }
  const uint64_t* run = run_score + o;
  if (threadIdx.x == 0) ctl->n_dst = 0;
  clear_hist<THR_NT>(hist);
  __syncthreads();
  Prefix pre;
  threshold_pass(run, n, pre, 0, nullptr, 0u, hist, ctl);
  __syncthreads();
  uint64_t m = n;  // candidates once they sit in LDS
  bool in_lds = false;
  uint32_t need = hi;
  for (int lvl = 0;; ++lvl) {
    find_pivot<THR_NT>(hist, need, ctl);
    const uint32_t pivot = ctl->pivot, pop = ctl->pop;
    need -= ctl->above;
    pre.push(level_of(lvl), pivot);
    if (lvl == THR_LEVELS - 1) break;
    const bool to_lds = !in_lds && pop <= (uint32_t)THR_CAND;
    __syncthreads();  // every thread has read ctl and the histogram
    clear_hist<THR_NT>(hist);
    if (threadIdx.x == 0) ctl->n_dst = 0;
    __syncthreads();
    if (in_lds) threshold_pass(cand, m, pre, lvl + 1, nullptr, 0u, hist, ctl);
    else threshold_pass(run, n, pre, lvl + 1, to_lds ? cand : nullptr, pop, hist, ctl);
    if (to_lds) { m = pop; in_lds = true; }
    __syncthreads();
  }
  if (threadIdx.x == 0) thr[q] = pre.s_val;  // all 63 score bits are pivot digits now
}

}  // namespace ps
