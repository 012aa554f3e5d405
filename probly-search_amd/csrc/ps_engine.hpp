// ps_engine.hpp — device side of a snapshot: HBM-resident CSR planes, per-batch plan upload,
// the scoring kernels and result download.  Implemented in ps_engine.hip (HIP, gfx950 only).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ps_snapshot.hpp"

// The handle behind the C ABI's ps_filter: a document allow-list resolved on one engine's device (Engine::filter_new).
struct ps_filter {
  uint64_t state = 0;           // the engine state it was made from (Engine: a process-wide serial, renewed by apply_delta)
  int device = -1;
  uint32_t* d_allow = nullptr;  // allow bitmap: alive AND listed, laid out and padded like the alive bitmap
  uint32_t* d_docs = nullptr;   // the allowed doc ids, ascending
  uint64_t len = 0;             // their number
};

// The handle behind the C ABI's ps_facet: one value id per document, resolved on one engine's device (Engine::facet_new).
struct ps_facet {
  uint64_t state = 0;          // the engine state it was made from, as ps_filter's
  int device = -1;
  uint16_t* d_col = nullptr;   // value + 1 per doc id (0 = none), padded like the alive bitmap
  uint32_t n_values = 0;
  uint64_t len = 0;            // alive documents that carry a value
};

namespace ps {

struct EngineImpl;

// Result records on their way to the C caller: a malloc'd block that grows without value-initialising
// (a full-result batch is hundreds of MB: every avoidable pass over it shows) and is handed over as it is.
// Large result blocks are PINNED host memory the device writes into directly (no pageable copy, whose first-touch
// page faults cost 17 ms for the 213 MB of a 24-query C2 batch); ps_free() hands such a block back to a process-wide
// pool instead of the allocator, the next batch reuses it (PS_RESULT_POOL_MB of idle blocks are kept, default 1024).
// result_block_release returns false for a pointer the pool does not know (then it is a malloc'd block).
void* result_block_acquire(size_t bytes, size_t* capacity);  // nullptr: no pinned memory to be had
bool result_block_release(void* p);

struct ResultBuf {
  ps_result* p = nullptr;
  size_t n = 0;
  size_t pinned_cap = 0;  // bytes of the pool block p points to, 0 = malloc'd
  ResultBuf() = default;
  ResultBuf(const ResultBuf&) = delete;
  ResultBuf& operator=(const ResultBuf&) = delete;
  ~ResultBuf() { drop(); }
  void drop() {
    if (pinned_cap) result_block_release(p); else free(p);
    p = nullptr;
    n = pinned_cap = 0;
  }
  void resize(size_t k) {
    const size_t bytes = (k ? k : 1) * sizeof(ps_result);
    if (pinned_cap) {
      if (bytes > pinned_cap) {  // grow: a larger pool block, or back to the allocator
        size_t cap = 0;
        void* q = result_block_acquire(bytes, &cap);
        if (!q) { q = malloc(bytes); cap = 0; }
        if (!q) throw std::bad_alloc();
        memcpy(q, p, n * sizeof(ps_result));
        result_block_release(p);
        p = static_cast<ps_result*>(q);
        pinned_cap = cap;
      }
      n = k;
      return;
    }
    void* q = realloc(p, bytes);
    if (!q) throw std::bad_alloc();
    p = static_cast<ps_result*>(q);
    n = k;
  }
  // k results in a pinned pool block when there is one to be had (contents undefined); false: malloc'd as resize()
  bool resize_pinned(size_t k) {
    drop();
    size_t cap = 0;
    void* q = result_block_acquire((k ? k : 1) * sizeof(ps_result), &cap);
    if (!q) { resize(k); return false; }
    p = static_cast<ps_result*>(q);
    pinned_cap = cap;
    n = k;
    return true;
  }
  void clear() { n = 0; }
  size_t size() const { return n; }
  ps_result* data() { return p; }
  ps_result& operator[](size_t i) { return p[i]; }
  void append(const ResultBuf& o) {
    const size_t at = n;
    resize(n + o.n);
    if (o.n) memcpy(p + at, o.p, o.n * sizeof(ps_result));
  }
  ps_result* release() {  // the caller's block now: ps_free() knows both kinds
    if (!p) resize(0);
    ps_result* r = p;
    p = nullptr;
    n = pinned_cap = 0;
    return r;
  }
};

class Engine {
 public:
  // Uploads the snapshot's planes to `device`.  Throws std::runtime_error on HIP failure.
  Engine(const Snapshot& snap, int device);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  // Runs one planned batch.  top_k == 0: every match (canonical order) into out/offsets.
  // top_k  > 0: the first top_k of the canonical order per query (up to PS_MAX_DEEP_TOPK selected on the device and
  // downloaded as a top-k block; beyond that the full result is sorted and cut).
  void run_host(const ps_scorer_desc& sc, const double* boosts, const Plan& plan, size_t top_k,
                ResultBuf& out, std::vector<size_t>& offsets, ps_batch_stats& stats, size_t skip = 0);
  // Device-resident top-k (1..PS_MAX_DEEP_TOPK) into caller buffers, ordered on `stream`
  // (nullptr = engine stream, synchronous).  Above PS_MAX_DEVICE_TOPK: the deep path - runs as in full-result mode,
  // then k_deep_select (ps_kernels_select.hpp), in slices of queries when the runs exceed PS_FULL_BUDGET_MB.
  // skip > 0 (both entries): ranks [skip, skip + top_k) instead of the first top_k - a result page, selected by
  // k_deep_window on that same path for every top_k in [1, PS_MAX_DEEP_TOPK]; skip + top_k <= 2^32 - 16.
  void run_device(const ps_scorer_desc& sc, const double* boosts, const Plan& plan, size_t top_k, void* d_keys,
                  void* d_scores, void* d_counts, void* stream, ps_batch_stats& stats, size_t skip = 0);

  // Exact total match counts - results.len() of Index::query (src/query.rs:97-105) - without scoring into runs, sorting
  // or downloading anything: Kc k_count_matches (ps_kernels_count.hpp) counts the union of the query's lists under the
  // alive bitmap where that is what "matches" means (BM25 with boosts >= 0, zero_to_one); any other scorer setting
  // takes stage 1 of the deep path and keeps its run lengths.  h_totals != nullptr: u64[B] on the host (synchronous,
  // engine stream); else d_totals, u64[B] on the device, ordered on `stream` (nullptr = engine stream, synchronous).
  void run_count(const ps_scorer_desc& sc, const double* boosts, const Plan& plan, void* d_totals, uint64_t* h_totals,
                 void* stream, ps_batch_stats& stats);

  // Resolves an allow-list of keys (any order, duplicates and unknown keys allowed) on the device: k_filter_build
  // (ps_kernels_filter.hpp).  Synchronous; the length comes down once.  A call that names the filter (ps_scorer_desc::filter)
  // is always planned on the host; it throws std::invalid_argument unless the filter was made by THIS engine in its current state.
  ps_filter* filter_new(const uint64_t* keys, size_t n_keys);

  // Resolves (key, value) pairs (any order, unknown keys ignored, the largest value of a repeated key) into a facet's
  // value column on the device: k_facet_build (ps_kernels_facet.hpp).  Synchronous; the length comes down once.  The
  // caller has checked values[i] < n_values <= PS_MAX_FACET_VALUES.
  ps_facet* facet_new(const uint64_t* keys, const uint32_t* values, size_t n, uint32_t n_values);
  // Facet counts - counts[q * n_values + v]: the documents of query q's full result list whose value is v - of a
  // host-planned batch: Kh k_facet_counts where run_count takes k_count_matches, stage 1 of the deep path and
  // Kr k_facet_runs where it takes the slow route.  h_counts / d_counts / stream as run_count's totals, u64[B * n_values].
  // Throws std::invalid_argument unless the facet was made by THIS engine in its current state.
  void run_facet_counts(const ps_scorer_desc& sc, const double* boosts, const Plan& plan, const ps_facet& facet, void* d_counts,
                        uint64_t* h_counts, void* stream, ps_batch_stats& stats);

  // SURVEY 8f N2 - device-side planner (BM25 and zero_to_one, built-in tokenizer): tokenise, term lookup in the frozen
  // trie, prefix expansion and before_each run on the GPU.  plan_device copies the plan back (tests);
  // run_device_planned scores the batch without the plan ever existing on the host.
  void plan_device(const char* text, const uint64_t* offsets, size_t n_queries, Plan& out);
  // Whether a flat BM25 top-k batch of this size (built-in tokenizer) should be planned on the device
  // (PS_DEVICE_PLAN, default on; small batches keep the host planner's latency path).
  bool wants_device_plan(size_t n_queries);
  // Announce the NEXT flat BM25 batch (ps_snapshot_plan_ahead_flat): its planner count pass starts now.
  bool plan_ahead(const ps_scorer_desc& sc, const char* text, const uint64_t* offsets, size_t n_queries);
  // false (top_k above PS_MAX_DEVICE_TOPK - the deep top-k path is planned on the host - and, zero_to_one only): the batch is not one K1dz takes (a query that is not simple, more than 4 lists, fewer
  // than PS_DAAT_MIN_BATCH queries ...) - nothing was enqueued, the caller plans it on the host.
  bool run_device_planned(const ps_scorer_desc& sc, const double* boosts, const char* text, const uint64_t* offsets,
                          size_t n_queries, size_t top_k, void* d_keys, void* d_scores, void* d_counts, void* stream,
                          ps_batch_stats& stats);

  // HIP-event durations summed over every batch since the last reset: the scoring kernel alone and
  // K0 / K0b in front of it (waits for outstanding launches).
  void kernel_times(ps_kernel_times& out, bool reset);
  // What the scoring kernels counted themselves (postings scanned, lookups by kind, ...) since the last reset.
  void work_counters(ps_work_counters& out, bool reset);
  // Device side of Snapshot::apply_delta: uploads exactly the ranges it changed (appended postings,
  // table entries, keys, alive words), drops what was derived from the old state and re-counts, on
  // the device, the per-layer pointer count of delta-removed documents.  Call with no batch in flight.
  void apply_delta(const DeltaRanges& r, std::vector<uint64_t>& removed_df, uint64_t* bytes_uploaded);
  uint64_t device_bytes() const;
  int device() const;

 private:
  EngineImpl* impl_;
};

void filter_free(ps_filter* f);  // (device memory: freed on the filter's device, whether or not its engine still exists)
void facet_free(ps_facet* f);    // (the same)
int device_count();
// Tuning knobs by name (the PS_* names of DESIGN.md section 11); read when a snapshot's engine is created.
void set_option(const char* name, uint32_t value);
bool get_option(const char* name, uint32_t* value);

}  // namespace ps
