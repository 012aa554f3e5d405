// ps_items.hpp - the K1d work-item rule in ONE place: how a list is cut into chunks and how many items it gets.  Used by the
// planner's count pass (ps_kernels_plan.hpp, k_plan), the host count of a host-planned batch (ps_engine.hip, count_daat_items),
// the preparation kernels (ps_prep_kernels.hpp: k_prep_query, k_prep_items, k_prep_tier_items) and K1dz's preparation
// (ps_z21_daat.hpp) - which must agree, or a launch sized from one of them skips items of another (FAULT_ITEM_COUNTS).
// Plain C++ (host and device): tests/c_abi/items_check.cpp prints it for tests/test_item_count_rule.py.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_ITEMS_HD __host__ __device__ __forceinline__
#else
#define PS_ITEMS_HD inline
#endif

namespace ps {

// Postings per item of a list of `len` postings: a split_div-th of the list rounded up to 256, at least chunk_min
// (PS_DAAT_SPLIT_DIV = 64: <= 64 chunks per list; PS_DAAT_CHUNK = 4096).
PS_ITEMS_HD uint32_t daat_chunk_of(const uint32_t split_div, const uint32_t chunk_min, const uint32_t len) {
  const uint32_t c = ((len + split_div - 1) / split_div + 255u) & ~255u;
  return c > chunk_min ? c : chunk_min;
}
// Items of a list cut into chunks of `chunk` postings (a tiered scan copy keeps a list's chunks whole: k_prep_tier_items).
PS_ITEMS_HD uint32_t daat_items_of(const uint32_t len, const uint32_t chunk) {
  return len == 0u ? 0u : (len + chunk - 1u) / chunk;
}

}  // namespace ps
