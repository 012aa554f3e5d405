// Prints the K1d work-item rule (csrc/ps_items.hpp) for the cases on the command line: one line "chunk items" per
// "len split_div chunk_min" triple.  Plain C++, no device: tests/test_item_count_rule.py compares it with a Python restatement.
#include <cstdio>
#include <cstdlib>

#include "../../probly-search_amd/csrc/ps_items.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const uint32_t len = (uint32_t)strtoul(argv[i], nullptr, 10), div = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
    const uint32_t cmin = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
    const uint32_t c = ps::daat_chunk_of(div, cmin, len);
    printf("%u %u\n", c, ps::daat_items_of(len, c));
  }
  return 0;
}
