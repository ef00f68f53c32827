"""The host side of the adaptive anti-aliasing pass (rt_antialias, rt_antialias_row_bands), without a GPU: the sub-pixel
grid of a level, the largest pass and the layout of the pass's one work allocation (tinyraytracerinrust_amd/csrc/
aa_plan.h, pure host code) in a stand-alone program built with the address and undefined-behaviour sanitizers, the
way tests/test_ray_paths_host.py tests paths_plan.h."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HARNESS = r"""
#include "aa_plan.h"
#include <cstdio>
#include <cstring>
using namespace rt;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void grids() {
  const int size[5] = {2, 3, 5, 9, 17};
  const size_t max_new[5] = {0, 5, 16, 56, 208};
  CHECK(RT_AA_MAX_LEVEL == 4 && RT_AA_HAVE_WORDS == 5);
  for (int level = 0; level <= RT_AA_MAX_LEVEL; ++level) {
    const AaPlan p = plan_aa(level, 1);
    CHECK(p.status == AaPlan::OK && p.size == size[level] && p.max_new == max_new[level] && p.cap == max_new[level]);
    CHECK((size_t)p.size * p.size <= 64 * RT_AA_HAVE_WORDS);          // a have bit per grid point
    const AaPlan none = plan_aa(level, 0);
    CHECK(none.status == AaPlan::NOTHING && none.size == size[level] && none.bytes == 0 && none.cap == 0);
  }
  printf("grids: %d failures\n", fails);
}

// the allocation as antialias_rows wrote it out before the plan existed
static size_t parent_bytes(int level, size_t n_edges) {
  const size_t sz = ((size_t)1 << level) + 1, per_col = sz * sz * 32, per_have = 5 * 8;
  size_t max_new = 0;
  for (int p = 1; p <= level; ++p) {
    const size_t a = ((size_t)1 << p) + 1, b = ((size_t)1 << (p - 1)) + 1;
    max_new = a * a - b * b > max_new ? a * a - b * b : max_new;
  }
  return n_edges * (per_col + per_have) + n_edges * max_new * 8 + 256;
}

static void layout() {
  const uint32_t edges[] = {1, 2, 63, 64, 65, 1000, 1u << 20, 8294400u};   // the last: every pixel of a 4K frame
  for (int level = 0; level <= RT_AA_MAX_LEVEL; ++level)
    for (uint32_t n : edges) {
      const AaPlan p = plan_aa(level, n);
      CHECK(p.status == AaPlan::OK);
      const size_t col_bytes = (size_t)n * p.size * p.size * RT_AA_COL_BYTES, have_bytes = (size_t)n * RT_AA_HAVE_WORDS * 8;
      CHECK(p.cap == (size_t)n * p.max_new);
      CHECK(p.col_off == 0 && p.col_off + col_bytes <= p.have_off);   // in order, none overlapping the next
      CHECK(p.have_off + have_bytes <= p.req_off);
      CHECK(p.req_off + p.cap * RT_AA_REQ_BYTES <= p.bytes);
      CHECK(p.col_off % 8 == 0 && p.have_off % 8 == 0 && p.req_off % 8 == 0);
      CHECK(p.bytes == parent_bytes(level, n));
      CHECK(p.have_off == col_bytes && p.req_off == col_bytes + have_bytes);   // ... and packed, as before
    }
  printf("layout: %d failures\n", fails);
}

static void too_many() {
  CHECK(plan_aa(0, 0xffffffffu).status == AaPlan::OK && plan_aa(0, 0xffffffffu).cap == 0);   // no pass, no request
  for (int level = 1; level <= RT_AA_MAX_LEVEL; ++level) {
    const uint64_t max_new = plan_aa(level, 1).max_new;
    const uint64_t first = 0xffffffffull / max_new + 1;             // the first n_edges with n_edges * max_new > 0xffffffff
    CHECK(first * max_new > 0xffffffffull && (first - 1) * max_new <= 0xffffffffull);
    if (first > 0xffffffffull) continue;
    const AaPlan last_ok = plan_aa(level, (uint32_t)(first - 1)), refused = plan_aa(level, (uint32_t)first);
    CHECK(last_ok.status == AaPlan::OK && last_ok.cap == (first - 1) * max_new && last_ok.bytes == parent_bytes(level, first - 1));
    CHECK(refused.status == AaPlan::TOO_MANY);
    CHECK(plan_aa(level, 0xffffffffu).status == AaPlan::TOO_MANY);
  }
  printf("too_many: %d failures\n", fails);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (!strcmp(argv[1], "grids")) grids();
  else if (!strcmp(argv[1], "layout")) layout();
  else if (!strcmp(argv[1], "too_many")) too_many();
  else return 2;
  return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which("g++"), "the library's own host compiler"
    d = tmp_path_factory.mktemp("aa_plan")
    (d / "h.cpp").write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-Wall", "-Wextra", f"-I{ROOT / 'tinyraytracerinrust_amd' / 'csrc'}", str(d / "h.cpp"),
                        "-o", str(d / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return d / "h"


def run(harness, section):
    r = subprocess.run([str(harness), section], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and f"{section}: 0 failures" in r.stdout


def test_grid_sizes_and_largest_pass(harness):
    """Levels 0..4: grids of 2, 3, 5, 9, 17 points a side, largest passes of 0, 5, 16, 56, 208 new points; no edge
    pixel: nothing to allocate."""
    run(harness, "grids")


def test_layout_is_ordered_aligned_and_the_former_size(harness):
    """Colour grids, have bits and request list follow one another without overlap, each 8-byte aligned, and the total
    is the formula antialias_rows used to write inline (the 256 spare bytes included), for 1, 65, 2^20 and more
    edge pixels at every level."""
    run(harness, "layout")


def test_too_many_from_the_first_overflowing_count(harness):
    """The request cap is refused exactly from the first edge count whose cap passes 32 bits (computed, per level;
    level 4: 20 648 882)."""
    run(harness, "too_many")
