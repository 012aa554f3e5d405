"""The K1d work-item rule lives in one header function (csrc/ps_items.hpp: daat_chunk_of / daat_items_of) that the planner's
count pass, the host count and the preparation kernels all call.  Here it is held against a plain Python restatement over a
table of (length, chunk rule) cases.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_of(length, split_div, chunk_min):
    """A split_div-th of the list, rounded up to a multiple of 256, at least chunk_min."""
    per = -(-length // split_div)
    return max(chunk_min, -(-per // 256) * 256)


def items_of(length, chunk):
    """ceil(length / chunk) chunks; no items for no postings."""
    return -(-length // chunk)


CASES = [(length, div, cmin)
         for cmin in (256, 300, 4096)
         for div in (1, 64)
         for length in (0, 1, 255, 256, 257, cmin - 1, cmin, cmin + 1, 2 * cmin, 64 * cmin - 1, 64 * cmin, 64 * cmin + 1, 65 * cmin,
                        100 * cmin + 7, 1_000_003, 33_353_544)]


def test_item_count_rule_matches_its_restatement(tmp_path):
    exe = str(tmp_path / "items_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c_abi", "items_check.cpp"), "-o", exe], check=True)
    args = [str(v) for case in CASES for v in case]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(CASES)
    for (length, div, cmin), line in zip(CASES, out):
        c, n = (int(v) for v in line.split())
        exp_c = chunk_of(length, div, cmin)
        assert (c, n) == (exp_c, items_of(length, exp_c)), (length, div, cmin, c, n)
    # the shapes the rule promises: one chunk exactly -> one item; a list of more than 64 minimum chunks -> at most 64 chunks
    assert items_of(4096, chunk_of(4096, 64, 4096)) == 1
    assert items_of(65 * 4096, chunk_of(65 * 4096, 64, 4096)) <= 64
