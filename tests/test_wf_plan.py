"""The wavefront launch's decisions (tinyraytracerinrust_amd/csrc/wf_plan.h: the counter block's names, the level
tables, the three arena layouts, plan_wavefront, the fold schedule, the pair lists' size) are pure host code; a
stand-alone program includes the header, is built with the address and undefined-behaviour sanitizers and checks
one section per test.  The layouts' and sizes' literals were obtained by evaluating the expressions of the commit
before wf_plan.h existed (k_wavefront.hip launch_wavefront / wfp_arena as of 8f6a077) for the same inputs."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HARNESS = r"""
#include "wf_plan.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
using namespace rt;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)

// fractal.scene's shape under the default options: a ray-tree scene of 171 objects, 2 lights, 1080p
static WfFacts base() {
  WfFacts f = {};
  f.n_tiles = 32400; f.max_depth = 10; f.f64 = false;
  f.cap_pct = 200; f.pairs_opt = 1; f.fast_clamp = true;
  f.shadow_pow = 1; f.n_objects = 171; f.n_lights = 2; f.n_trav = 300;
  f.any_transparent = true; f.colour_fast = true;
  return f;
}

static void counters() {
  std::set<int> words;
  int n = 0;
  auto add = [&](int w) { CHECK(w >= 0 && w < RT_WF_COUNT_WORDS); words.insert(w); ++n; };
  for (int d = 0; d <= RT_MAX_DEPTH_CAP + 1; ++d) {
    add(WFC_LEVEL + d);
    CHECK(WFC_LEVEL + d < WFC_OVERFLOW && WFC_LEVEL + d < WFC_PAIRS);
  }
  add(WFC_OVERFLOW);
  CHECK(WFC_OVERFLOW < WFC_PAIRS);
  for (int w : {WFP_NEAREST, WFP_SHADOW, WFP_WRAPPED, WFP_NEED, WFP_WRAP}) add(WFC_PAIRS + w);
  for (int d = 0; d <= RT_WFP_LOG_LEVELS; ++d) { add(WFC_PAIRS + wfp_log(d, false)); add(WFC_PAIRS + wfp_log(d, true)); }
  CHECK((int)words.size() == n);                              // all distinct
  CHECK(RT_WF_COUNT_WORDS == 64);
  // the values the kernels were written against
  CHECK(WFC_OVERFLOW == RT_MAX_DEPTH_CAP + 2 && WFC_PAIRS == 32 && RT_WFP_LOG_LEVELS == 12);
  CHECK(WFP_NEAREST == 0 && WFP_SHADOW == 1 && WFP_WRAPPED == 2 && WFP_NEED == 3 && WFP_WRAP == 4);
  CHECK(wfp_log(0, false) == 5 && wfp_log(0, true) == 6 && wfp_log(12, true) == 30);
  CHECK(WFP_WRAP == WFP_NEED + 1);                            // the host reads the two sticky words in one copy
}

struct Region { size_t begin, bytes, align; };
static void regions_ok(const std::vector<Region>& r, size_t total) {
  size_t end = 0;
  for (const Region& q : r) {
    CHECK(q.begin >= end);                                    // disjoint, in order
    CHECK(q.begin % q.align == 0);
    end = q.begin + q.bytes;
  }
  CHECK(end <= total);
}
static long layout_case(size_t tiles, int pct, int depth, int lights) {
  WfFacts f = base();
  f.n_tiles = tiles; f.cap_pct = pct; f.max_depth = depth; f.n_lights = lights;
  const WfPlan p = plan_wavefront(f);
  CHECK(!p.refused);
  const size_t S = p.slots, C = p.cap, R = p.rays, nl = (size_t)std::max(1, lights);
  CHECK(R == std::max(S, C));
  // the level arena: level tables (doubles then words, per level), counters, flags, kout, perm, sort scratch
  std::vector<Region> a;
  for (int d = 0; d <= depth; ++d) {
    const size_t len = d == 0 ? S : C, off = wf_level_offset(S, C, d);
    const int nf = d == 0 ? WF_N_F64 - WF_F64_0 : (int)WF_N_F64, nw = d == 0 ? WF_I32_0_END - WF_I32_0 : (int)WF_N_I32;
    for (int k = 0; k < nf; ++k) a.push_back({off + (size_t)k * len * 8, len * 8, 8});
    for (int k = 0; k < nw; ++k) a.push_back({off + (size_t)nf * len * 8 + (size_t)k * len * 4, len * 4, 4});
    CHECK(off + len * (d == 0 ? RT_WF_BYTES0 : RT_WF_BYTES) == wf_level_offset(S, C, d + 1));
  }
  a.push_back({p.arena.count, 256, 256});
  a.push_back({p.arena.ovf, S, 1});
  a.push_back({p.arena.kout, C * 4, 256});
  a.push_back({p.arena.perm, C * 4, 4});
  a.push_back({p.arena.tmp, RT_WF_LEVEL_BINS * 4, 256});
  regions_ok(a, p.arena.bytes);
  // the pair path's per-ray block
  const WfRayLayout& r = p.ray;
  regions_ok({{r.tmin, R * 8, 256}, {r.omin, R * 4, 256}, {r.px, 3 * R * 8, 256}, {r.kcnt, R * nl * 4, 256},
              {r.opq, R * nl * 4, 256}, {r.hkey, 4 * R * 4, 256}}, r.bytes);
  CHECK(r.bytes % 256 == 0);
  // the pair lists at their first size
  const WfListSize s = wf_list_size(0, C, 0);
  CHECK(s.grow && !s.refused && s.cap % 64 == 0);
  const WfListLayout l = wf_list_layout(s.cap);
  regions_ok({{l.bins, 3 * RT_WFP_BIN_WORDS * 4, 256}, {l.key, 4 * s.cap * 4, 4}, {l.tp, s.cap * 8, 8}}, l.bytes);
  CHECK(l.bytes % 256 == 0);
  return 1;
}
static bool arena_is(const WfPlan& p, size_t count, size_t ovf, size_t kout, size_t perm, size_t tmp, size_t bytes) {
  const WfArenaLayout& a = p.arena;
  return a.count == count && a.ovf == ovf && a.kout == kout && a.perm == perm && a.tmp == tmp && a.bytes == bytes;
}
static bool ray_is(const WfPlan& p, std::vector<size_t> v) {
  const WfRayLayout& r = p.ray;
  return std::vector<size_t>{r.tmin, r.omin, r.px, r.kcnt, r.opq, r.hkey, r.bytes} == v;
}
static bool list_is(size_t cap, std::vector<size_t> v) {
  const WfListLayout l = wf_list_layout(cap);
  return std::vector<size_t>{l.bins, l.key, l.tp, l.bytes} == v;
}
static long layouts() {
  long n = 0;
  for (size_t tiles : {(size_t)1, (size_t)2, (size_t)70, (size_t)32400})
    for (int pct : {1, 50, 100, 200, 333})
      for (int depth : {0, 1, 6, RT_MAX_DEPTH_CAP})
        for (int lights : {0, 1, 3}) n += layout_case(tiles, pct, depth, lights);
  CHECK(RT_WF_BYTES0 == 48 && RT_WF_BYTES == 112);
  CHECK(wf_level_offset(64, 128, 0) == 0 && wf_level_offset(64, 128, 1) == 3072 && wf_level_offset(64, 128, 3) == 3072 + 2 * 128 * 112);
  // literals: (tiles, percent, depth, lights) -> slots, cap, the arena's and the per-ray block's offsets and totals
  auto plan = [](size_t tiles, int pct, int depth, int lights) {
    WfFacts f = base();
    f.n_tiles = tiles; f.cap_pct = pct; f.max_depth = depth; f.n_lights = lights;
    return plan_wavefront(f);
  };
  WfPlan p = plan(1, 200, 0, 0);
  CHECK(p.slots == 64 && p.cap == 128 && arena_is(p, 3072, 3328, 3584, 4096, 4608, 21248));
  CHECK(ray_is(p, {0, 1024, 1536, 4608, 5120, 5632, 7680}));
  p = plan(1, 1, 16, 3);                                      // cap at its floor
  CHECK(p.slots == 64 && p.cap == 64 && arena_is(p, 117760, 118016, 118272, 118528, 118784, 135424));
  CHECK(ray_is(p, {0, 512, 768, 2304, 3072, 3840, 4864}));
  p = plan(70, 200, 6, 2);                                    // 75 x 50
  CHECK(p.slots == 4480 && p.cap == 8960 && arena_is(p, 6236160, 6236416, 6241024, 6276864, 6312704, 6329344));
  CHECK(ray_is(p, {0, 71680, 107520, 322560, 394240, 465920, 609280}));
  p = plan(70, 1, 6, 2);
  CHECK(p.slots == 4480 && p.cap == 64 && arena_is(p, 258048, 258304, 262912, 263168, 263424, 280064));
  CHECK(ray_is(p, {0, 35840, 53760, 161280, 197120, 232960, 304640}));
  p = plan(32400, 200, 10, 2);                                // 1080p
  CHECK(p.slots == 2073600 && p.cap == 4147200 &&
        arena_is(p, 4744396800ull, 4744397056ull, 4746470656ull, 4763059456ull, 4779648256ull, 4779664896ull));
  CHECK(ray_is(p, {0, 33177600, 49766400, 149299200, 182476800, 215654400, 282009600}));
  CHECK(list_is(64, {0, 49152, 50176, 50688}));
  CHECK(list_is(256, {0, 49152, 53248, 55296}));
  CHECK(list_is(4147200, {0, 49152, 66404352, 99581952}));
  return n;
}

static void plan() {
  WfFacts f;
  WfPlan p;
  // RT_OPT_WAVEFRONT_PAIRS 0 / 1 / 2 -> first pair level none / 1 / 0
  f = base(); f.pairs_opt = 0; p = plan_wavefront(f);
  CHECK(p.first_pair_level == -1 && !p.pairs_level(0) && !p.pairs_level(1) && !p.pairs_level(16));
  f.pairs_opt = 1; p = plan_wavefront(f);
  CHECK(p.first_pair_level == 1 && !p.pairs_level(0) && p.pairs_level(1) && p.pairs_level(16));
  f.pairs_opt = 2; p = plan_wavefront(f);
  CHECK(p.first_pair_level == 0 && p.pairs_level(0) && p.pairs_level(1));
  // each of the pair path's conditions at its boundary
  f = base(); f.shadow_pow = 0;
  CHECK(plan_wavefront(f).first_pair_level == -1);
  f = base(); f.n_objects = 0;
  CHECK(plan_wavefront(f).first_pair_level == -1);
  f.n_objects = 1;
  CHECK(plan_wavefront(f).first_pair_level == 1);
  f.n_objects = 4095;
  CHECK(plan_wavefront(f).first_pair_level == 1);
  f.n_objects = 4096;
  CHECK(plan_wavefront(f).first_pair_level == -1);
  // the shadow-ray ids: max(slots, cap) x max(1, lights) < 2^32.  Both factors' first is a multiple of 64, so the
  // largest product below 2^32 is 2^32 - 64 = 64 x 22369621 x 3
  f = base(); f.cap_pct = 1; f.n_tiles = 22369621; f.n_lights = 3; p = plan_wavefront(f);
  CHECK(!p.refused && (uint64_t)p.rays * 3 == (1ull << 32) - 64 && p.first_pair_level == 1);
  f.n_tiles = (size_t)1 << 24; f.n_lights = 4; p = plan_wavefront(f);
  CHECK(!p.refused && (uint64_t)p.rays * 4 == (1ull << 32) && p.first_pair_level == -1);
  f.n_lights = 3;
  CHECK(plan_wavefront(f).first_pair_level == 1);
  f = base(); f.cap_pct = 1; f.n_tiles = ((size_t)1 << 25) - 1; f.n_lights = 0; p = plan_wavefront(f);   // no light: one id per ray
  CHECK(!p.refused && p.rays == (1ull << 31) - 64 && p.first_pair_level == 1);
  f = base(); f.n_tiles = (size_t)1 << 23; f.cap_pct = 300; f.n_lights = 3; p = plan_wavefront(f);          // cap is the larger
  CHECK(!p.refused && p.rays == p.cap && p.cap == 3 * ((size_t)1 << 29) && p.first_pair_level == -1);
  f.n_lights = 2;
  CHECK(plan_wavefront(f).first_pair_level == 1);
  // the kernels' flags
  f = base(); p = plan_wavefront(f);
  CHECK(p.refr && p.fc && !p.f64 && p.max_depth == 10);
  f.any_transparent = false; f.f64 = true;
  CHECK(!plan_wavefront(f).refr && plan_wavefront(f).f64);
  f = base(); f.fast_clamp = false;
  CHECK(!plan_wavefront(f).fc);
  f = base(); f.colour_fast = false;
  CHECK(!plan_wavefront(f).fc);
  // the hierarchy in LDS: up to 1280 nodes, never in a diagnostic build that says so
  f = base(); f.n_trav = 1280; p = plan_wavefront(f);
  CHECK(p.lds_trav && p.trav_lds == 1280 * sizeof(RtTravC) && p.trav_lds == 40960);
  f.n_trav = 1281; p = plan_wavefront(f);
  CHECK(!p.lds_trav && p.trav_lds == 0);
  f.n_trav = 1280; f.global_trav = true;
  CHECK(!plan_wavefront(f).lds_trav);
  // the candidate kernels count their pairs for the fused-scan sorts: up to 2048 objects
  f = base(); f.n_objects = 2048; p = plan_wavefront(f);
  CHECK(p.counted && p.hist_lds == 2048 * 4);
  f.n_objects = 2049; p = plan_wavefront(f);
  CHECK(!p.counted && p.hist_lds == 0);
  // the hit-point key's cell bits
  f = base(); f.n_objects = 1;
  CHECK(plan_wavefront(f).cbits == 10);
  f.n_objects = 171;
  CHECK(plan_wavefront(f).cbits == 3);
  f.n_objects = 2047;
  CHECK(plan_wavefront(f).cbits == 0);
  for (int nobj = 1; nobj < 4096; ++nobj) {                   // the sort's bins fit the fused scan where any bit is used
    f.n_objects = nobj;
    const int cb = plan_wavefront(f).cbits;
    CHECK(cb >= 0 && cb <= 12 && (cb == 0 || ((uint32_t)(nobj + 1) << cb) <= RT_BS_FUSED_BINS));
    CHECK(cb == 12 || ((uint32_t)(nobj + 1) << (cb + 1)) > RT_BS_FUSED_BINS);
  }
  // the capacity: percent of the slots, in whole waves, one wave at least
  for (size_t tiles : {(size_t)1, (size_t)3, (size_t)70, (size_t)32400, (size_t)129600})
    for (int pct = 1; pct <= 400; ++pct) {
      f = base(); f.n_tiles = tiles; f.cap_pct = pct; p = plan_wavefront(f);
      const size_t want = tiles * 64 * (size_t)pct / 100;
      CHECK(!p.refused && p.slots == tiles * 64 && p.cap % 64 == 0 && p.cap >= 64);
      CHECK(p.cap >= want && (p.cap == 64 || p.cap - want < 64));
    }
  f = base(); f.n_tiles = 1; f.cap_pct = 1;
  CHECK(plan_wavefront(f).cap == 64);
  f.n_tiles = 70; f.cap_pct = 200;
  CHECK(plan_wavefront(f).cap == 8960);
  // 2^31 - 1 slots or rays per level at most
  f = base(); f.cap_pct = 100; f.n_tiles = ((size_t)1 << 25) - 1; p = plan_wavefront(f);
  CHECK(!p.refused && p.slots == (1ull << 31) - 64 && p.cap == p.slots);
  f.n_tiles = (size_t)1 << 25; p = plan_wavefront(f);
  CHECK(p.refused && !strcmp(p.error, "wavefront launch of 2147483648 pixel slots too large"));
  f = base(); f.cap_pct = 200; f.n_tiles = (size_t)1 << 24; p = plan_wavefront(f);   // the capacity alone
  CHECK(p.refused && !strcmp(p.error, "wavefront launch of 1073741824 pixel slots too large"));
  f.n_tiles = ((size_t)1 << 24) - 1; p = plan_wavefront(f);
  CHECK(!p.refused && p.cap == (1ull << 31) - 128);
}

static void folds() {
  for (int last = 0; last <= RT_MAX_DEPTH_CAP + 1; ++last) {
    const WfFolds s = wf_fold_schedule(last);
    const int top = std::max(last - 1, 0);
    std::vector<int> covered(top + 1, 0);
    CHECK(s.n >= 1 && s.n <= (int)(sizeof s.step / sizeof s.step[0]));
    for (int k = 0; k < s.n; ++k) {
      CHECK(s.step[k].span >= 1 && s.step[k].span <= RT_WF_FOLD_SPAN);
      CHECK(s.step[k].d >= 0 && s.step[k].d + s.step[k].span - 1 <= top);
      for (int d = s.step[k].d; d < s.step[k].d + s.step[k].span && d <= top; ++d) ++covered[d];
      if (k > 0) CHECK(s.step[k].d + s.step[k].span == s.step[k - 1].d);      // descending, no gap
    }
    CHECK(s.step[0].d + s.step[0].span - 1 == top);
    CHECK(s.step[s.n - 1].d == 0);
    for (int c : covered) CHECK(c == 1);
  }
  auto is = [](int last, std::vector<std::pair<int, int>> want) {
    const WfFolds s = wf_fold_schedule(last);
    if (s.n != (int)want.size()) return false;
    for (int k = 0; k < s.n; ++k)
      if (s.step[k].d != want[k].first || s.step[k].span != want[k].second) return false;
    return true;
  };
  CHECK(RT_WF_FOLD_SPAN == 3);                                // (what the literals below assume)
  CHECK(is(0, {{0, 1}}) && is(1, {{0, 1}}));
  CHECK(is(2, {{0, 2}}));
  CHECK(is(3, {{0, 3}}));
  CHECK(is(4, {{1, 3}, {0, 1}}));
  CHECK(is(6, {{3, 3}, {0, 3}}));
  CHECK(is(17, {{14, 3}, {11, 3}, {8, 3}, {5, 3}, {2, 3}, {0, 2}}));
}

static void lists() {
  auto is = [](size_t have, size_t lcap, size_t need, bool grow, size_t cap) {
    const WfListSize s = wf_list_size(have, lcap, need);
    return s.grow == grow && !s.refused && s.cap == cap;
  };
  // the first size: 4 pairs per ray of a full level, in whole waves
  CHECK(is(0, 64, 0, true, 256));
  CHECK(is(0, 100, 0, true, 448));
  CHECK(is(0, 8960, 0, true, 35840));
  CHECK(is(0, 4147200, 0, true, 16588800));
  // lists that hold what is needed stay
  CHECK(is(256, 64, 0, false, 256) && is(256, 64, 256, false, 256) && is(35840, 8960, 1000, false, 35840));
  // growth: a quarter beyond the need, never below the first size
  CHECK(is(256, 64, 257, true, 384));
  CHECK(is(256, 64, 1000, true, 1280) && is(256, 64, 1001, true, 1280));
  CHECK(is(35840, 8960, 1000000, true, 1250048));
  CHECK(is(256, 8960, 300, true, 35840));
  // the ceiling
  CHECK(is(256, 64, 1717986816ull, true, 2147483520ull));
  CHECK(is(256, 64, 1717986918ull, true, 0x7fffffc0ull));
  CHECK(is(256, 64, 0x7fffffc0ull, true, 0x7fffffc0ull));
  WfListSize s = wf_list_size(256, 64, 0x7fffffc1ull);
  CHECK(s.grow && s.refused && !strcmp(s.error, "wavefront pair list of 2147483585 pairs too large"));
  s = wf_list_size(0x7fffffc0ull, 64, 0xffffffffull);         // the most a 32-bit sticky word can ask for
  CHECK(s.refused && !strcmp(s.error, "wavefront pair list of 4294967295 pairs too large"));
}

int main(int argc, char** argv) {
  const char* what = argc > 1 ? argv[1] : "";
  long n = 0;
  if (!strcmp(what, "counters")) counters();
  else if (!strcmp(what, "layouts")) n = layouts();
  else if (!strcmp(what, "plan")) plan();
  else if (!strcmp(what, "folds")) folds();
  else if (!strcmp(what, "lists")) lists();
  else return 2;
  printf("%s: %d failures, %ld cases\n", what, fails, n);
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("wf_plan")
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
    return int(r.stdout.split()[-2])


def test_counter_block(harness):
    """Every named word of the 64-word counter block is distinct and below 64; the level counts reach neither the
    overflow word nor the pair block; the log words of levels 0..RT_WFP_LOG_LEVELS fit."""
    run(harness, "counters")


def test_layouts(harness):
    """The level arena, the pair path's per-ray block and the pair lists over a grid of (tiles, percent, depth,
    lights) that includes 1 tile, the capacity's floor of 64, depth 0 and RT_MAX_DEPTH_CAP: regions disjoint and in
    order, doubles 8-aligned, words 4-aligned, the counter block and the rounded regions 256-aligned; five sizes'
    offsets and totals as literals."""
    assert run(harness, "layouts") == 4 * 5 * 4 * 3


def test_plan(harness):
    """The pair path's five conditions each at its boundary, the first pair level per option value, lds_trav at
    1280 / 1281 nodes, counted at 2048 / 2049 objects, cbits for 1 / 171 / 2047 objects, the capacity rule, the
    2^31 refusals and their messages."""
    run(harness, "plan")


def test_fold_schedule(harness):
    """For every last level 0..RT_MAX_DEPTH_CAP + 1 the folds cover levels 0..max(last - 1, 0) once, descending,
    within RT_WF_FOLD_SPAN levels each, the last from level 0; six schedules as literals."""
    run(harness, "folds")


def test_pair_list_size(harness):
    """The first size, growth to need + need / 4, the 0x7fffffc0 ceiling, the refusal beyond it."""
    run(harness, "lists")
