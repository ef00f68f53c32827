"""The launches' decisions (tinyraytracerinrust_amd/csrc/launch_plan.h: band_geometry, clamp_bands, plan_row_launch,
order_from_costs) are pure host code; a stand-alone program includes the header, is built with the address and
undefined-behaviour sanitizers and checks one section per test: the rule table of the kernel choice, the
plan's invariants over the product of its inputs, the tile orders on the smallest vectors that take each
branch, the band checks' messages, and the side entries' clamped layouts.  The GPU tests pin the same choices
end to end through rt_ctx_kernel_info."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HARNESS = r"""
#include "launch_plan.h"
#include <cstdio>
#include <cstring>
#include <set>
using namespace rt;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)
static const int TRCAP = 128, SPLIT_LOG2 = 3;
static const uint32_t TILE_MASK = 0xFFFFFu;

// a reflection-only scene of 8 objects under the default options, 30000 tiles, no order slot, no program
static LaunchFacts base() {
  LaunchFacts f = {};
  f.colour_fast = true; f.n_lights = 2; f.n_objects = 8;
  f.kernel_opt = RT_KERNEL_AUTO; f.tile_order = true; f.tile_masks = 1; f.tile_records = f.sky_fill = f.fast_clamp = true;
  f.sky_ok = f.masks_ok = true;
  f.max_depth = 5; f.n_tiles = 30000; f.slot = LaunchFacts::NONE;
  f.sh_trcap = TRCAP; f.split_tile_mask = TILE_MASK; f.refl_pooled = false; f.pool_byte_index = true;
  return f;
}
static LaunchFacts chain_scene() { LaunchFacts f = base(); f.any_transparent = f.ray_chains = true; return f; }
static LaunchFacts tree_scene() { LaunchFacts f = base(); f.any_transparent = true; return f; }
// ... with the scene's single-scene program loaded, every row kind present
static LaunchFacts spec(LaunchFacts f) {
  f.loaded = true;
  f.mode = f.any_transparent ? (f.ray_chains ? RT_MODE_CHAIN : RT_MODE_TREE) : RT_MODE_REFL;
  f.fc = f.colour_fast && f.fast_clamp;
  f.has[SPEC_ROWS] = f.has[SPEC_DEFERRED] = f.has[SPEC_PRIMARY] = f.has[SPEC_ROWS_NOMASK] = f.has_rows_ordered = true;
  return f;
}
static LaunchFacts slot(LaunchFacts f, LaunchFacts::Slot s, bool deferred = false, bool masks_pay = false, int wf_tune = 0) {
  f.slot = s; f.slot_deferred = deferred; f.masks_pay = masks_pay; f.wf_tune = wf_tune;
  return f;
}
static bool is(const LaunchPlan& p, LaunchPlan::Path path, const char* last, int kind = -1) {
  return p.path == path && !strcmp(p.last_kernel, last) && p.kind == kind;
}

static void table() {
  LaunchFacts f;
  // 1, 2: reflection-only, fewer than RT_ORDER_MIN_TILES tiles
  f = base(); f.n_tiles = RT_ORDER_MIN_TILES - 1;
  CHECK(is(plan_row_launch(f), LaunchPlan::DEFERRED, "deferred"));
  f.kernel_opt = RT_KERNEL_MEGA;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel"));
  f = base(); f.tile_order = false;                      // (tile order off: by the tile count)
  CHECK(plan_row_launch(f).path == LaunchPlan::DEFERRED);
  f.n_tiles = RT_DEFERRED_MAX_TILES;
  CHECK(plan_row_launch(f).path == LaunchPlan::MEGA);
  // 3: calibrating, whatever the slot later says
  CHECK(is(plan_row_launch(slot(base(), LaunchFacts::CALIBRATING, true)), LaunchPlan::MEGA, "megakernel"));
  // 4: ordered: the slot's choice
  CHECK(is(plan_row_launch(slot(base(), LaunchFacts::ORDERED, true)), LaunchPlan::DEFERRED, "deferred"));
  CHECK(is(plan_row_launch(slot(base(), LaunchFacts::ORDERED, false)), LaunchPlan::MEGA, "megakernel"));
  // 5: refraction chains: never under auto, only on request
  f = chain_scene(); f.n_tiles = 100;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel"));
  CHECK(plan_row_launch(slot(chain_scene(), LaunchFacts::ORDERED, true)).path == LaunchPlan::MEGA);
  f.kernel_opt = RT_KERNEL_DEFERRED;
  CHECK(is(plan_row_launch(f), LaunchPlan::DEFERRED, "deferred") && plan_row_launch(f).chain && plan_row_launch(f).mode == RT_MODE_CHAIN);
  f = tree_scene(); f.kernel_opt = RT_KERNEL_DEFERRED;   // (ray trees: no deferred kernel at all)
  CHECK(plan_row_launch(f).path == LaunchPlan::MEGA && plan_row_launch(f).mode == RT_MODE_TREE);
  // 6: too many tiles for an order entry, or too many lights: not even on request
  f = base(); f.kernel_opt = RT_KERNEL_DEFERRED; f.n_tiles = (size_t)TILE_MASK + 1;
  CHECK(plan_row_launch(f).path == LaunchPlan::DEFERRED && plan_row_launch(f).defer_forced);
  f.n_tiles = (size_t)TILE_MASK + 2;
  CHECK(plan_row_launch(f).path == LaunchPlan::MEGA && !plan_row_launch(f).defer_forced);
  f = base(); f.kernel_opt = RT_KERNEL_DEFERRED; f.n_lights = TRCAP;
  CHECK(plan_row_launch(f).path == LaunchPlan::DEFERRED);
  f.n_lights = TRCAP + 1;
  CHECK(plan_row_launch(f).path == LaunchPlan::MEGA);
  // 7: ray trees, ordered: tune / megakernel / wavefront
  LaunchPlan p = plan_row_launch(slot(tree_scene(), LaunchFacts::ORDERED, false, false, 0));
  CHECK(is(p, LaunchPlan::MEGA, "megakernel") && p.tune);
  p = plan_row_launch(slot(tree_scene(), LaunchFacts::ORDERED, false, false, 1));
  CHECK(is(p, LaunchPlan::MEGA, "megakernel") && !p.tune);
  p = plan_row_launch(slot(tree_scene(), LaunchFacts::ORDERED, false, false, 2));
  CHECK(is(p, LaunchPlan::WAVEFRONT, "wavefront") && !p.tune);
  CHECK(!plan_row_launch(slot(tree_scene(), LaunchFacts::CALIBRATING)).tune);
  f = slot(tree_scene(), LaunchFacts::ORDERED); f.kernel_opt = RT_KERNEL_MEGA;
  CHECK(!plan_row_launch(f).tune);
  CHECK(!plan_row_launch(slot(chain_scene(), LaunchFacts::ORDERED)).tune && !plan_row_launch(slot(base(), LaunchFacts::ORDERED)).tune);
  // 8: the wavefront path on request
  f = spec(base()); f.kernel_opt = RT_KERNEL_WAVEFRONT;
  p = plan_row_launch(f);
  CHECK(is(p, LaunchPlan::WAVEFRONT, "wavefront") && !p.masks && !p.records && !p.sky && !p.tune);
  // 9: max_depth 0 with a primary kernel loaded clears `deferred`, unless deferred was requested
  f = spec(base()); f.max_depth = 0; f.n_tiles = 100;
  CHECK(is(plan_row_launch(f), LaunchPlan::PRIMARY, "primary-ray (specialised)", SPEC_PRIMARY));
  CHECK(is(plan_row_launch(slot(f, LaunchFacts::ORDERED, true)), LaunchPlan::PRIMARY, "primary-ray (specialised)", SPEC_PRIMARY));
  f.kernel_opt = RT_KERNEL_DEFERRED;
  CHECK(is(plan_row_launch(f), LaunchPlan::DEFERRED, "deferred (specialised)", SPEC_DEFERRED));
  f = spec(base()); f.max_depth = 0; f.has[SPEC_PRIMARY] = false;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel (specialised)", SPEC_ROWS_NOMASK));
  f = base(); f.max_depth = 0;                           // (no program: the generic megakernel)
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel"));
  // 10: the program's mode or clamp form is not the launch's: generic
  f = spec(base()); f.mode = RT_MODE_CHAIN;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel"));
  f = spec(base()); f.fast_clamp = false;                // the launch's fc is now false, the program's true
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel") && !plan_row_launch(f).fc);
  f = spec(base()); f.n_tiles = 100; f.has[SPEC_DEFERRED] = false;   // (a program without the kind)
  CHECK(is(plan_row_launch(f), LaunchPlan::DEFERRED, "deferred"));
  // 11: a family program, or more than 32 objects: no masks
  const LaunchFacts ordered_pay = slot(spec(base()), LaunchFacts::ORDERED, false, true);
  p = plan_row_launch(ordered_pay);
  CHECK(is(p, LaunchPlan::MEGA, "megakernel (specialised)", SPEC_ROWS) && p.masks);
  f = ordered_pay; f.family = true;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel (specialised)", SPEC_ROWS_NOMASK) && !plan_row_launch(f).masks);
  f = ordered_pay; f.n_objects = 33;
  CHECK(!plan_row_launch(f).masks);
  f.n_objects = 32;
  CHECK(plan_row_launch(f).masks);
  f = ordered_pay; f.masks_ok = false;
  CHECK(!plan_row_launch(f).masks);
  CHECK(!plan_row_launch(slot(spec(chain_scene()), LaunchFacts::ORDERED, false, true)).masks);
  // 12: RT_OPT_TILE_MASKS 0 / 1 / 2
  const LaunchFacts prim = [] { LaunchFacts g = spec(base()); g.max_depth = 0; return g; }();
  for (int tm = 0; tm < 3; ++tm) {
    auto masks = [&](LaunchFacts g) { g.tile_masks = tm; return plan_row_launch(g).masks; };
    CHECK(masks(ordered_pay) == (tm >= 1));                                            // ordered, masks pay
    CHECK(masks(slot(spec(base()), LaunchFacts::ORDERED, false, false)) == (tm == 2)); // ordered, they do not
    CHECK(masks(prim) == (tm >= 1));                                                   // primary rays: always
    CHECK(masks(slot(prim, LaunchFacts::CALIBRATING)) == (tm >= 1));
    CHECK(masks(slot(spec(base()), LaunchFacts::CALIBRATING, false, true)) == (tm == 2));   // calibrating
    LaunchFacts un = spec(base()); un.tile_order = false; un.n_tiles = 50000;          // unordered megakernel
    CHECK(plan_row_launch(un).path == LaunchPlan::MEGA && masks(un) == (tm == 2));
    CHECK(!masks(slot(spec(base()), LaunchFacts::ORDERED, true, true)));               // the deferred kernel: never
  }
  // 13: records only with a table, RT_OPT_TILE_RECORDS on and a non-deferred slot
  CHECK(plan_row_launch(ordered_pay).records);
  f = ordered_pay; f.tile_records = false;
  CHECK(plan_row_launch(f).masks && !plan_row_launch(f).records);
  f = ordered_pay; f.tile_masks = 0;
  CHECK(!plan_row_launch(f).records);
  p = plan_row_launch(slot(prim, LaunchFacts::ORDERED, true, false));   // primary rays over a deferred slot's split entries
  CHECK(p.path == LaunchPlan::PRIMARY && p.masks && !p.records && !p.sky);
  // 14: sky only with records, not calibrating, and sky_fill && sky_ok
  CHECK(plan_row_launch(ordered_pay).sky);
  f = ordered_pay; f.sky_fill = false;
  CHECK(plan_row_launch(f).records && !plan_row_launch(f).sky);
  f = ordered_pay; f.sky_ok = false;
  CHECK(plan_row_launch(f).records && !plan_row_launch(f).sky);
  f = ordered_pay; f.tile_records = false;
  CHECK(!plan_row_launch(f).sky);
  f = slot(spec(base()), LaunchFacts::CALIBRATING); f.tile_masks = 2;
  CHECK(plan_row_launch(f).records && !plan_row_launch(f).sky);
  // 15: no table: the mask-free megakernel when the program has one
  f = slot(spec(base()), LaunchFacts::ORDERED, false, false);
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel (specialised)", SPEC_ROWS_NOMASK));
  f.has[SPEC_ROWS_NOMASK] = false;
  CHECK(is(plan_row_launch(f), LaunchPlan::MEGA, "megakernel (specialised)", SPEC_ROWS));
  // 16: a pooled kernel and more than 256 objects
  f = chain_scene(); f.n_objects = 257;
  CHECK(plan_row_launch(f).refused);
  f.n_objects = 256;
  CHECK(!plan_row_launch(f).refused);
  f.n_objects = 257; f.kernel_opt = RT_KERNEL_DEFERRED;  // (the deferred kernel has no pool)
  CHECK(plan_row_launch(f).path == LaunchPlan::DEFERRED && !plan_row_launch(f).refused);
  f = base(); f.n_objects = 257;
  CHECK(!plan_row_launch(f).refused);
  f.refl_pooled = true;
  CHECK(plan_row_launch(f).refused);
  f = tree_scene(); f.n_objects = 257;
  CHECK(!plan_row_launch(f).refused);
  // two-eye scenes: the view megakernel whatever the options say
  f = spec(base()); f.views = true; f.kernel_opt = RT_KERNEL_WAVEFRONT;
  CHECK(is(plan_row_launch(f), LaunchPlan::VIEWS, "view megakernel"));
  f.two_eyes = f.has[SPEC_VIEWS] = true;
  CHECK(is(plan_row_launch(f), LaunchPlan::VIEWS, "view megakernel (specialised)", SPEC_VIEWS) && !plan_row_launch(f).masks);
  f = chain_scene(); f.views = true; f.n_objects = 257;
  CHECK(plan_row_launch(f).refused);
  // what the calibration is told: the tail decides for the generic kernels only, below RT_DEFERRED_MAX_TILES
  CHECK(plan_row_launch(slot(base(), LaunchFacts::CALIBRATING)).defer_if_tail);
  CHECK(!plan_row_launch(slot(spec(base()), LaunchFacts::CALIBRATING)).defer_if_tail);
  f = slot(base(), LaunchFacts::CALIBRATING); f.n_tiles = RT_DEFERRED_MAX_TILES;
  CHECK(!plan_row_launch(f).defer_if_tail);
  CHECK(!plan_row_launch(slot(chain_scene(), LaunchFacts::CALIBRATING)).defer_if_tail);
}

static long invariants() {
  long n = 0;
  const int kopts[] = {RT_KERNEL_AUTO, RT_KERNEL_MEGA, RT_KERNEL_DEFERRED, RT_KERNEL_WAVEFRONT};
  const size_t tiles[] = {100, 30000, (size_t)TILE_MASK + 2};
  for (int scene = 0; scene < 3; ++scene) for (int cf = 0; cf < 2; ++cf) for (int no : {8, 33})
  for (int ko : kopts) for (int to = 0; to < 2; ++to) for (int tm = 0; tm < 3; ++tm) for (int tr = 0; tr < 2; ++tr)
  for (int sky = 0; sky < 4; ++sky) for (int mok = 0; mok < 2; ++mok) for (int md : {0, 5}) for (size_t nt : tiles)
  for (int sl = 0; sl < 3; ++sl) for (int sd = 0; sd < (sl == 2 ? 2 : 1); ++sd) for (int mp = 0; mp < (sl == 2 ? 2 : 1); ++mp)
  for (int wt = 0; wt < (sl == 2 && scene == 2 ? 3 : 1); ++wt)
  for (int prog = 0; prog < 4; ++prog)                   // none, the scene's, another mode's, the scene's family program
  for (int has = 0; has < (prog ? 16 : 1); ++has) {
    if (sl && (!to || nt < RT_ORDER_MIN_TILES || ko == RT_KERNEL_WAVEFRONT)) continue;   // such launches have no slot
    LaunchFacts f = base();
    f.any_transparent = scene != 0; f.ray_chains = scene == 1; f.colour_fast = cf; f.n_objects = no;
    f.kernel_opt = ko; f.tile_order = to; f.tile_masks = tm; f.tile_records = tr; f.sky_fill = sky & 1; f.sky_ok = sky >> 1;
    f.masks_ok = mok; f.max_depth = md; f.n_tiles = nt;
    f = slot(f, (LaunchFacts::Slot)sl, sd, mp, wt);
    if (prog) {
      f = spec(f);
      if (prog == 2) f.mode = (f.mode + 1) % 3;
      f.family = prog == 3;
      f.has[SPEC_ROWS] = has & 1; f.has[SPEC_DEFERRED] = has & 2; f.has[SPEC_PRIMARY] = has & 4; f.has[SPEC_ROWS_NOMASK] = has & 8;
    }
    const LaunchPlan p = plan_row_launch(f);
    ++n;
    CHECK(!p.records || p.masks);
    CHECK(!p.sky || p.records);
    // masks: a specialised non-deferred reflection megakernel, or the primary kernel -- of a scene that has a table
    CHECK(!p.masks || (p.kind == SPEC_ROWS && p.path == LaunchPlan::MEGA && p.mode == RT_MODE_REFL) ||
          (p.kind == SPEC_PRIMARY && p.path == LaunchPlan::PRIMARY && p.mode == RT_MODE_REFL));
    CHECK(!p.masks || (f.masks_ok && f.tile_masks && f.n_objects <= 32 && !f.family));
    CHECK(p.kind != SPEC_ROWS_NOMASK || !p.masks);
    CHECK(p.kind < 0 || (f.loaded && f.has[p.kind]));
    CHECK((p.path == LaunchPlan::PRIMARY) == (p.kind == SPEC_PRIMARY));
    CHECK(p.path != LaunchPlan::DEFERRED || (scene != 2 && nt <= (size_t)TILE_MASK + 1 && (scene == 0 || ko == RT_KERNEL_DEFERRED)));
    CHECK(p.path != LaunchPlan::WAVEFRONT || (!p.masks && !p.records && !p.sky && !p.tune && p.kind < 0));
    CHECK(p.path != LaunchPlan::VIEWS);
    CHECK(!p.tune || (scene == 2 && sl == 2 && ko == RT_KERNEL_AUTO));
    if (fails > 20) return n;
  }
  return n;
}

// a deferred order's entries -> per tile its parts, checked; returns the tiles in first-part order
static std::vector<int> split_tiles(const std::vector<int32_t>& e, size_t n_tiles) {
  std::vector<int> tiles;
  std::set<int> seen;
  for (size_t i = 0; i < e.size();) {
    const int t = e[i] & (int)TILE_MASK, lp = (e[i] >> 24) & 15;
    CHECK(lp <= SPLIT_LOG2 && (size_t)t < n_tiles && seen.insert(t).second);
    for (int part = 0; part < (1 << lp); ++part, ++i)    // the parts of one tile: adjacent, numbered 0 .. 2^lp - 1
      CHECK(i < e.size() && e[i] == (int32_t)((uint32_t)t | (uint32_t)part << 20 | (uint32_t)lp << 24));
    tiles.push_back(t);
  }
  CHECK(tiles.size() == n_tiles);
  return tiles;
}
static bool longest_first(const std::vector<int>& tiles, const std::vector<uint32_t>& cost) {
  for (size_t i = 1; i < tiles.size(); ++i) {
    const uint32_t a = cost[tiles[i - 1]], b = cost[tiles[i]];
    if (a < b || (a == b && tiles[i - 1] > tiles[i])) return false;   // index order kept among equals
  }
  return true;
}

static void orders() {
  const OrderParams plain = {8.0, false, false, SPLIT_LOG2, false, 0, 0};   // launch_views' call: no split, no XCD order
  // eight tiles with ties
  TileOrder o = order_from_costs({5, 9, 5, 0, 9, 5, 7, 0}, plain);
  CHECK((o.entries == std::vector<int32_t>{1, 4, 6, 0, 2, 5, 3, 7}) && !o.deferred);
  // a 16 x 4-tile grid with one dominant tile and few slots: the tail decides
  std::vector<uint32_t> cost(64, 100);
  cost[37] = 100000; cost[3] = 450; cost[60] = 250; cost[12] = 199; cost[13] = 200;
  OrderParams tail = plain;
  tail.defer_if_tail = true;
  o = order_from_costs(cost, tail);
  CHECK(o.deferred && !o.masks_pay);
  const std::vector<int> tiles = split_tiles(o.entries, 64);
  CHECK(longest_first(tiles, cost));
  CHECK(o.entries.size() == 64 + 7 + 3 + 1 + 1);         // 100000: 8 parts; 450: 4; 250 and 200: 2 (cost >= P x the median 100)
  CHECK(o.entries[0] == (int32_t)(37u | 0u << 20 | 3u << 24) && o.entries[8] == (int32_t)(3u | 0u << 20 | 2u << 24));
  o = order_from_costs(cost, plain);                     // the same costs where the plan leaves no choice: not deferred
  CHECK(!o.deferred && !o.masks_pay && o.entries.size() == 64 && o.entries[0] == 37);
  OrderParams forced = plain;
  forced.defer_forced = true;
  // flat costs: throughput-bound
  o = order_from_costs(std::vector<uint32_t>(64, 100), tail);
  CHECK(!o.deferred && o.masks_pay && o.entries.size() == 64 && o.entries[0] == 0 && o.entries[63] == 63);
  o = order_from_costs(std::vector<uint32_t>(8, 100), tail);      // costliest tile == the work per slot: not a tail yet
  CHECK(!o.deferred && o.masks_pay);
  o = order_from_costs({101, 100, 100, 100, 100, 100, 100, 99}, tail);
  CHECK(o.deferred && !o.masks_pay);
  o = order_from_costs(std::vector<uint32_t>(64, 100), forced);   // on request: deferred, nothing to split
  CHECK(o.deferred && o.masks_pay && o.entries.size() == 64 && split_tiles(o.entries, 64).size() == 64);
  o = order_from_costs(std::vector<uint32_t>(64, 0), forced);     // (no tile stored a cost: the median counts as 1)
  CHECK(o.deferred && o.entries.size() == 64);
  // the XCD line order on 32 x 2 tiles, lines of 4 tiles
  std::vector<uint32_t> c2(64);
  for (int t = 0; t < 64; ++t) c2[t] = (uint32_t)((t * 37) % 64) * 10 + 1;   // distinct
  OrderParams xcd = plain;
  xcd.xcd = true; xcd.tiles_x = 32; xcd.line_tiles = 4;
  o = order_from_costs(c2, xcd);
  CHECK(!o.deferred && std::set<int32_t>(o.entries.begin(), o.entries.end()).size() == 64 && o.entries.size() == 64);
  uint32_t prev = ~0u;
  for (int block = 0; block < 2; ++block)
    for (int e = 0; e < 8; ++e) {
      const int32_t* b = &o.entries[block * 32];
      uint32_t line_cost = 0;
      for (int j = 0; j < 4; ++j) {                      // one line's four tiles sit at e, e + 8, e + 16, e + 24
        CHECK(b[e + 8 * j] == b[e] + j && b[e] % 4 == 0);
        line_cost = std::max(line_cost, c2[b[e + 8 * j]]);
      }
      CHECK(line_cost < prev);                           // lines by their costliest tile
      prev = line_cost;
    }
  xcd.defer_forced = true;                               // a deferred order takes no line order
  o = order_from_costs(c2, xcd);
  CHECK(o.deferred && longest_first(split_tiles(o.entries, 64), c2));
  // splitting off: a plain permutation, longest first
  o = order_from_costs(c2, plain);
  CHECK(o.entries.size() == 64 && longest_first(std::vector<int>(o.entries.begin(), o.entries.end()), c2));
}

static bool rejected(const BandGeometry& g, const char* msg) { return g.status == BandGeometry::REJECTED && !strcmp(g.error, msg); }
static void geometry() {
  BandGeometry g = band_geometry(65, 48, 8, 3, 5, 3);
  CHECK(g.status == BandGeometry::OK && g.n_rows == 9 && g.tiles_x == (65 + RT_TILE_W - 1) / RT_TILE_W);
  CHECK(g.tiles_y == (9 + 64 / RT_TILE_W - 1) / (64 / RT_TILE_W) && g.n_tiles == (size_t)g.tiles_x * g.tiles_y);
  CHECK(band_geometry(64, 48, 0, 0, 4, 2).status == BandGeometry::NOTHING);      // zero rows, zero bands: nothing to do
  CHECK(band_geometry(64, 48, 0, 4, 4, 0).status == BandGeometry::NOTHING);
  CHECK(!strcmp(band_geometry(64, 48, 0, 4, 4, 0).error, "no rows"));            // (the mask calls' message for it)
  CHECK(band_geometry(64, 48, 99, 0, 0, 0).status == BandGeometry::NOTHING);     // (ahead of every other check)
  CHECK(rejected(band_geometry(64, 48, 0, 4, 2, 2), "band pitch 2 < band rows 4"));
  CHECK(band_geometry(64, 48, 0, 4, 2, 1).status == BandGeometry::OK);           // one band: the pitch is not read
  CHECK(rejected(band_geometry(64, 48, 48, 4, 4, 1), "first row 48 >= height 48"));
  CHECK(band_geometry(64, 48, 47, 4, 4, 1).status == BandGeometry::OK);
  CHECK(rejected(band_geometry(64, 48, 0, 4096, 4096, 4097), "too many rows"));
  CHECK(rejected(band_geometry(64, 48, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu), "too many rows"));
  g = band_geometry(64, 48, 0, 4096, 4096, 4096);                                // 2^24 rows: the limit itself
  CHECK(g.status == BandGeometry::OK && g.n_rows == (1u << 24));
  CHECK(rejected(band_geometry(64, 48, 4000000000u, 4000000000u, 3, 2), "band pitch 3 < band rows 4000000000"));
}

// The side entries' band rule.  band_row is rt_bodies.h's formula, restated here (device code is not included):
// which frame row the kernels read packed row r of the clamped layout from.
static uint32_t band_row(const BandGeometry& g, uint32_t r) {
  return g.band_rows >= g.n_rows ? g.y_first + r : g.y_first + (r / g.band_rows) * g.band_pitch + r % g.band_rows;
}
static long clamp() {
  long accepted = 0;
  // every accepted layout: the kernels' packed rows are exactly the caller's rows below H, at the caller's packed
  // places (band b row j at b * band_rows + j), in order
  for (int H = 1; H <= 13; ++H) for (uint32_t y0 = 0; y0 <= 14; ++y0) for (uint32_t br = 0; br <= 5; ++br)
  for (uint32_t bp = 0; bp <= 7; ++bp) for (uint32_t nb = 0; nb <= 4; ++nb) {
    const BandGeometry g = clamp_bands(65, H, y0, br, bp, nb);
    if (br == 0 || nb == 0) { CHECK(g.status == BandGeometry::NOTHING); continue; }
    if (bp < br && nb > 1) { CHECK(g.status == BandGeometry::REJECTED); continue; }
    if (y0 >= (uint32_t)H) { CHECK(g.status == BandGeometry::REJECTED); continue; }
    CHECK(g.status == BandGeometry::OK && g.n_rows > 0);
    if (g.status != BandGeometry::OK) continue;
    ++accepted;
    uint32_t r = 0;
    bool same = true;
    for (uint32_t b = 0; b < nb; ++b)
      for (uint32_t j = 0; j < br; ++j) {
        const uint32_t y = y0 + b * bp + j;
        if (y >= (uint32_t)H) continue;
        same = same && r < g.n_rows && r == b * br + j && band_row(g, r) == y;
        ++r;
      }
    CHECK(same && r == g.n_rows);
    CHECK(g.tiles_x == 9 && g.tiles_y == (int)(g.n_rows + 7) / 8 && g.n_tiles == (size_t)g.tiles_x * g.tiles_y);
    if (fails > 20) return accepted;
  }
  // the three statuses, both messages, and the order of the checks (as band_geometry's)
  CHECK(clamp_bands(64, 48, 0, 0, 4, 2).status == BandGeometry::NOTHING);
  CHECK(clamp_bands(64, 48, 0, 4, 4, 0).status == BandGeometry::NOTHING);
  CHECK(clamp_bands(64, 48, 99, 0, 0, 0).status == BandGeometry::NOTHING);       // (ahead of every other check)
  CHECK(!strcmp(clamp_bands(64, 48, 0, 4, 4, 0).error, "no rows"));
  CHECK(rejected(clamp_bands(64, 48, 0, 4, 2, 2), "band pitch 2 < band rows 4"));
  CHECK(rejected(clamp_bands(64, 48, 99, 4, 2, 2), "band pitch 2 < band rows 4"));   // (ahead of the first row's)
  CHECK(clamp_bands(64, 48, 0, 4, 2, 1).status == BandGeometry::OK);             // one band: the pitch is not read
  CHECK(rejected(clamp_bands(64, 48, 48, 4, 4, 1), "first row 48 >= height 48"));
  CHECK(rejected(clamp_bands(64, 48, 4000000000u, 4000000000u, 3, 2), "band pitch 3 < band rows 4000000000"));
  // rt_antialias' call: one band of more rows than any frame has
  for (int H : {1, 7, 48, 65535}) {
    const BandGeometry g = clamp_bands(64, H, 0, UINT32_MAX, UINT32_MAX, 1);
    CHECK(g.status == BandGeometry::OK && g.y_first == 0 && g.band_rows == (uint32_t)H && g.band_pitch == (uint32_t)H && g.n_rows == (uint32_t)H);
  }
  // more bands than any frame has, from the last row: one row
  BandGeometry g = clamp_bands(64, 48, 47, 1, 1, UINT32_MAX);
  CHECK(g.status == BandGeometry::OK && g.y_first == 47 && g.band_rows == 1 && g.band_pitch == 1 && g.n_rows == 1);
  // a cut layout as the kernels receive it: rows 3-6, 11-14, 19-20 of 21
  g = clamp_bands(41, 21, 3, 4, 8, 5);
  CHECK(g.status == BandGeometry::OK && g.y_first == 3 && g.band_rows == 4 && g.band_pitch == 8 && g.n_rows == 10);
  CHECK(band_row(g, 3) == 6 && band_row(g, 4) == 11 && band_row(g, 9) == 20);
  // the 8x8 tiles of a 65-wide, 9-row layout
  g = clamp_bands(65, 48, 8, 3, 5, 3);
  CHECK(g.status == BandGeometry::OK && g.n_rows == 9 && g.tiles_x == 9 && g.tiles_y == 2 && g.n_tiles == 18);
  CHECK(RT_TILE_W == 8);                                                         // (what the literals above assume)
  return accepted;
}

int main(int argc, char** argv) {
  const char* what = argc > 1 ? argv[1] : "";
  long n = 0;
  if (!strcmp(what, "table")) table();
  else if (!strcmp(what, "invariants")) n = invariants();
  else if (!strcmp(what, "orders")) orders();
  else if (!strcmp(what, "geometry")) geometry();
  else if (!strcmp(what, "clamp")) n = clamp();
  else return 2;
  printf("%s: %d failures, %ld cases\n", what, fails, n);
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("launch_plan")
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


def test_plan_table(harness):
    """One row per rule of the kernel choice as launch_plan.h's comments state them: facts -> path, catalogue
    kind, rt_ctx_kernel_info's words, masks / records / sky, the ray-tree tune, the pooled-kernel refusal."""
    run(harness, "table")


def test_plan_invariants(harness):
    """Over the product of the plan's inputs: records imply masks, sky implies records, a table goes only to a
    specialised non-deferred reflection megakernel or the primary-ray kernel of a scene that has one, a
    launched kind is one the program holds."""
    assert run(harness, "invariants") > 100000


def test_order_from_costs(harness):
    """Ties keep index order; a dominant tile with few wave slots gives a deferred order of split parts; flat
    costs do not; the XCD line order; launch_views' plain permutation."""
    run(harness, "orders")


def test_band_geometry(harness):
    """Every rejected band launch keeps its message; 2^24 rows pass, one more does not; zero rows or bands
    are reported as nothing to do."""
    run(harness, "geometry")


def test_clamp_bands(harness):
    """The side entries' band rule over H 1..13, y_first 0..14, band_rows 0..5, band_pitch 0..7, n_bands 0..4:
    every accepted layout's packed rows are, through the kernels' band_row, exactly the caller's rows below H at
    the caller's packed places, and there is at least one; the statuses and messages; rt_antialias' one huge band."""
    assert run(harness, "clamp") >= 10000
