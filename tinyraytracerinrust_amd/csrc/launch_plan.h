// launch_plan.h -- every decision of a launch as pure host code: plain C++17, no HIP header and no
// rt_device.h, so tests/test_launch_plan.py compiles and runs it on a CPU.  Four functions:
//   band_geometry     the row and band checks and the tile arithmetic of a row launch
//   clamp_bands       the same checks (band_checks) for a side entry, and the layout cut to the rows that exist
//   plan_row_launch   which kernel a launch runs, and what it is handed (masks, records, sky fill)
//   order_from_costs  a calibration's tile costs -> the dispatch order and the slot's two choices
// Two band rules, because two kinds of kernel read a layout.  The row launches (k_rows.hip launch_bands, k_stereo.hip
// launch_views, k_masks.hip) keep the caller's layout as it is -- band_geometry: their tile orders, masks and
// records are keyed by it, and the render kernels drop the rows >= H themselves.  The side entries (k_aa.hip
// antialias_rows, k_stats.hip rt_count_rays_row_bands, k_hits.hip rt_first_hits_row_bands) stage and copy back exactly n_rows packed rows, so
// the host cuts the layout first -- clamp_bands: bands that start at or past H go, the last band ends at H.
// The callers see rt_device.h and pass its constants in (rt_ctx.hip finish_calibration among them).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "spec.h"   // the kernel catalogue (SpecKind); rt_blob.h's RT_TILE_W and RT_MODE_*, rt_abi.h's RT_KERNEL_*

// Launches with fewer tiles than this are dispatched row-major without a calibration launch: a
// small band (a single row, one rank's sliver) has no tail worth reordering, and calibrating it
// would cost a host synchronisation per new geometry.
#ifndef RT_ORDER_MIN_TILES
#define RT_ORDER_MIN_TILES 2048
#endif

// Kernel choice for scenes without a transparent object (REFR = false), RT_OPT_KERNEL AUTO:
//   * launches of fewer than RT_ORDER_MIN_TILES tiles (no calibration) take the deferred kernel;
//   * larger launches calibrate on the megakernel; the ordered launches that follow take the
//     deferred kernel with split tiles when the launch has fewer than RT_DEFERRED_MAX_TILES tiles
//     AND its costliest tile is longer than the work per wave slot (sum of tile costs / the chip's
//     wave slots for the calibrated kernel: CUs x 4 SIMDs x its waves per SIMD): then the tail,
//     not the throughput, sets the time.
// Same pixels either way.  Measured (profiles/r02h_inflight.txt, r02j_*): a rank's share of the
// 4K globes frame at N = 8 / 4 (16320 / 32640 tiles, tail ratio 3.5 / 1.8) takes 0.146-0.178 /
// 0.187-0.204 ms deferred + split against 0.244 / 0.254 ms in the megakernel, 1080p globes d5
// (ratio 1.7) 0.219 against 0.26-0.28 ms; at N = 2 / 1 (64800 / 129600 tiles, ratio 1.0 / 0.5),
// and for the 1080p single sphere (32400 tiles, ratio 0.75: no tail to speak of), the megakernel
// is 7-20 % faster.  The deferred kernel's order entries hold the tile index in 20 bits
// (RT_SPLIT_TILE_MASK), so launches of more tiles always take the megakernel.
#define RT_DEFERRED_MAX_TILES 40000

// RT_OPT_TRACED_MASKS 1: the row launches an upload must have had before a launch takes a traced table
// (plan_row_launch below).
#ifndef RT_TRACED_MIN_LAUNCHES
#define RT_TRACED_MIN_LAUNCHES 8
#endif

namespace rt {

// ---- band_geometry, clamp_bands ------------------------------------------------------------------------
struct BandGeometry {
  enum { OK = 0, NOTHING, REJECTED } status;   // NOTHING: zero rows or zero bands (the launches: RT_OK; the mask calls fail)
  char error[64];                              // not OK: the message (RT_ERR_INVALID); NOTHING: "no rows"
  uint32_t y_first, band_rows, band_pitch, n_rows;   // OK: the layout the kernels receive, and its 8x8 tiles
  int tiles_x, tiles_y;
  size_t n_tiles;
};

// The checks the two rules share, in this order; true: the layout passed them (g is not accepted yet).
inline bool band_checks(BandGeometry& g, int height, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands) {
  g = {};
  g.status = BandGeometry::REJECTED;
  if (band_rows == 0 || n_bands == 0) { g.status = BandGeometry::NOTHING; snprintf(g.error, sizeof g.error, "no rows"); }
  else if (band_pitch < band_rows && n_bands > 1) snprintf(g.error, sizeof g.error, "band pitch %u < band rows %u", band_pitch, band_rows);
  else if (y_first >= (uint32_t)height) snprintf(g.error, sizeof g.error, "first row %u >= height %d", y_first, height);
  else return true;
  return false;
}
inline void band_accept(BandGeometry& g, int width, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_rows) {
  const uint32_t tile_h = 64 / RT_TILE_W;      // rt_device.h RT_TILE_H
  g.status = BandGeometry::OK;
  g.y_first = y_first; g.band_rows = band_rows; g.band_pitch = band_pitch; g.n_rows = n_rows;
  g.tiles_x = (width + RT_TILE_W - 1) / RT_TILE_W;
  g.tiles_y = (int)((n_rows + tile_h - 1) / tile_h);
  g.n_tiles = (size_t)g.tiles_x * (size_t)g.tiles_y;
}

// A row launch: the caller's layout as it is, at most 2^24 packed rows.
inline BandGeometry band_geometry(int width, int height, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch,
                                  uint32_t n_bands) {
  BandGeometry g;
  if (!band_checks(g, height, y_first, band_rows, band_pitch, n_bands)) return g;
  const uint64_t rows = (uint64_t)band_rows * n_bands;
  if (rows > (1u << 24)) snprintf(g.error, sizeof g.error, "too many rows");
  else band_accept(g, width, y_first, band_rows, band_pitch, (uint32_t)rows);
  return g;
}

// A side entry: the bands that start below H, the last of them cut to H; a single band becomes (y_first, rows, rows).
// Every packed row r < n_rows then exists: rt_bodies.h band_row(r) < H.
inline BandGeometry clamp_bands(int width, int height, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch,
                                uint32_t n_bands) {
  BandGeometry g;
  if (!band_checks(g, height, y_first, band_rows, band_pitch, n_bands)) return g;
  const uint32_t H = (uint32_t)height;
  if (n_bands > 1) n_bands = std::min(n_bands, (H - 1 - y_first) / band_pitch + 1);
  const uint32_t last_rows = std::min(band_rows, H - (y_first + (n_bands - 1) * band_pitch));
  if (n_bands == 1) band_rows = band_pitch = last_rows;
  band_accept(g, width, y_first, band_rows, band_pitch, (n_bands - 1) * band_rows + last_rows);
  return g;
}

// ---- plan_row_launch ----------------------------------------------------------------------------------
struct LaunchFacts {
  // the uploaded scene (RtDevScene)
  bool any_transparent, ray_chains, colour_fast;
  int n_lights, n_objects;
  bool views;                     // a two-eye scene: the view megakernel, nothing else
  // the context's options
  int kernel_opt;                 // RT_KERNEL_*
  bool tile_order;
  int tile_masks;                 // RT_OPT_TILE_MASKS 0 / 1 / 2
  bool tile_records, sky_fill, fast_clamp;
  // what the upload found
  bool sky_ok, masks_ok;
  // the launch
  int max_depth;
  bool f64;
  size_t n_tiles;
  // its order slot
  enum Slot { NONE = 0, CALIBRATING, ORDERED } slot;
  bool slot_deferred, masks_pay;
  int wf_tune;                    // OrderSlot::wf_tune
  // the loaded specialised program, and which catalogue kinds have a function for this (f64, cal)
  bool loaded;
  int mode;
  bool fc, family, two_eyes;
  bool has[SPEC_KINDS];
  bool has_rows_ordered;          // SPEC_ROWS for (f64, cal = false): what a calibrating launch's successors would run
  // rt_device.h's constants
  int sh_trcap;                   // RT_SH_TRCAP
  uint32_t split_tile_mask;       // RT_SPLIT_TILE_MASK
  bool refl_pooled;               // RT_LDS_POOL_REFL > 0
  bool pool_byte_index;           // RT_POOL_OBJ_INDEX
  // lean tiles: RT_OPT_LEAN_TILES, and the program holds the lean kernel for this f64 and its check
  bool lean_tiles = false, has_lean = false;
  // traced tile masks: RT_OPT_TRACED_MASKS 0 / 1 / 2 / 3, and the program holds the pass (the check kernel: has_check)
  int traced_masks = 0;
  bool has_check = false;
  uint32_t launches_since_upload = 0;   // row launches of this context since rt_ctx_upload, this one not counted
};

struct LaunchPlan {
  enum Path { WAVEFRONT = 0, MEGA, DEFERRED, PRIMARY, VIEWS } path;
  int mode;                       // RT_MODE_* of the scene
  bool chain, fc;                 // the generic kernels' remaining template flags
  bool tune;                      // time this launch against the wavefront path (ray trees, once per geometry)
  int kind;                       // the catalogue kind to launch, -1: the generic kernel
  bool masks, records;            // fill (ahead of the timing event) AND pass the mask table / the dispatch records:
                                  // one boolean each, so what is filled is what the kernel reads
  bool sky;                       // the records may say sky
  bool refused;                   // a pooled kernel for more than 256 objects
  const char* last_kernel;        // rt_ctx_kernel_info's words
  // for the calibration this launch ends with (order_from_costs)
  bool defer_forced, defer_if_tail;
  // the records carry checked lean bits, and the program's lean kernel runs ahead of the megakernel
  bool lean = false;
  // the records' words come from the trace pass (rt_bodies.h trace_masks_body), which also sets the lean bits
  bool traced = false;
  // ... and the pass also traces the entries with a pixel on a boxed object and flags them (RT_OPT_TRACED_MASKS 1 / 3)
  bool traced_objects = false;
};

inline LaunchPlan plan_row_launch(const LaunchFacts& f) {
  LaunchPlan p = {};
  p.kind = -1;
  const bool refr = f.any_transparent, chain = refr && f.ray_chains, tree = refr && !chain;
  const bool calibrate = f.slot == LaunchFacts::CALIBRATING, ordered = f.slot == LaunchFacts::ORDERED;
  p.mode = chain ? RT_MODE_CHAIN : refr ? RT_MODE_TREE : RT_MODE_REFL;
  p.chain = chain;
  p.fc = f.colour_fast && f.fast_clamp;
  const bool match = f.loaded && p.mode == f.mode && p.fc == f.fc;   // the context holds a program for this launch
  // Two encodings in these kernels name an object in fewer bits than an int: the wave pool's frames hold
  // the hit object in ONE BYTE (rt_device.h RT_POOL_OBJ_INDEX: chain kernels, and reflection-only builds
  // with a pool) and the tile masks hold one BIT per object in a 32-bit word (rt_tilemask.h).  Both
  // limits are checked here, where such a kernel is chosen: a pooled kernel is refused beyond 256
  // objects (flatten already keeps such scenes out of the chain mode), a masked one takes no table
  // beyond 32 (put_mask_scene marks such scenes, and the specialised programs stop at 32 objects too).
  const bool pooled_mode = p.mode == RT_MODE_CHAIN || (p.mode == RT_MODE_REFL && f.refl_pooled);
  // A two-eye scene: always the view megakernel of the scene's mode, generic or specialised.
  if (f.views) {
    p.path = LaunchPlan::VIEWS;
    if (match && f.two_eyes && f.has[SPEC_VIEWS]) p.kind = SPEC_VIEWS;
    p.last_kernel = p.kind >= 0 ? "view megakernel (specialised)" : "view megakernel";
    p.refused = pooled_mode && f.pool_byte_index && f.n_objects > 256;
    return p;
  }
  p.last_kernel = "wavefront";
  if (f.kernel_opt == RT_KERNEL_WAVEFRONT) return p;
  // Kernel choice for scenes without a transparent object (RT_DEFERRED_MAX_TILES): the per-lane
  // megakernel is fastest when the launch fills the GPU many times over (throughput-bound); a
  // launch bound by its costliest tiles' latency takes the deferred-shadow kernel with split
  // costly tiles (DESIGN.md "Deferred shadows").  An ordered launch takes its slot's choice.
  // The deferred kernel takes scenes whose rays form chains (reflection-only, or refraction chains);
  // the library's own choice (AUTO) takes it for reflection-only scenes only: on refraction chains it
  // measured 3.2x slower than the chain megakernel (spinning_globes 1080p lone frame 0.80 vs 0.25 ms,
  // profiles/r03b_chain_ab.txt), so there it runs only when RT_KERNEL_DEFERRED asks for it.
  const bool eligible = (!refr || chain) && f.n_lights <= f.sh_trcap && f.n_tiles <= (size_t)f.split_tile_mask + 1;
  const bool auto_ok = eligible && !refr;
  // -1 auto, 0 megakernel, 1 deferred (the context's RT_OPT_KERNEL)
  const int dmode = f.kernel_opt == RT_KERNEL_MEGA ? 0 : f.kernel_opt == RT_KERNEL_DEFERRED ? 1 : -1;
  bool deferred;
  if (!eligible || dmode == 0) deferred = false;
  else if (dmode == 1) deferred = true;
  else if (!auto_ok) deferred = false;
  else if (ordered) deferred = f.slot_deferred;
  else if (calibrate) deferred = false;                       // calibrate on the megakernel
  else deferred = f.n_tiles < RT_ORDER_MIN_TILES || (!f.tile_order && f.n_tiles < RT_DEFERRED_MAX_TILES);
  // Ray-tree scenes (a transparent AND reflective object) under RT_KERNEL_AUTO: the first ordered
  // launch of a geometry is timed against one wavefront launch of the same rows, and the faster
  // path takes every later launch (fractal.scene 1080p: 16.4 vs 25.9 ms, profiles/r03d_timing.txt;
  // the small ray-tree scenes of the fuzz suite mostly keep the megakernel).  Same pixels either way.
  if (ordered && tree && f.wf_tune == 2) return p;
  p.tune = ordered && tree && dmode == -1 && f.wf_tune == 0;
  // launches of primary rays only (max_depth 0) take the program's primary-ray kernel (no frame stack,
  // rt_device.h PRIM) unless the deferred kernel was asked for
  const bool prim = match && f.max_depth == 0 && dmode != 1 && f.has[SPEC_PRIMARY];
  if (prim) deferred = false;
  p.path = prim ? LaunchPlan::PRIMARY : deferred ? LaunchPlan::DEFERRED : LaunchPlan::MEGA;
  const int kind = prim ? SPEC_PRIMARY : deferred ? SPEC_DEFERRED : SPEC_ROWS;
  if (match && f.has[kind]) p.kind = kind;
  p.last_kernel = prim ? "primary-ray (specialised)"
                       : deferred ? (p.kind >= 0 ? "deferred (specialised)" : "deferred")
                                  : (p.kind >= 0 ? "megakernel (specialised)" : "megakernel");
  p.refused = !deferred && pooled_mode && f.pool_byte_index && f.n_objects > 256;
  // The launch geometry's tile masks: the single-scene reflection-only programs' megakernel and
  // primary-ray kernel read them (a family program, the other modes and the deferred kernel take none).
  // RT_OPT_TILE_MASKS 1: the primary-ray kernel always takes the table (its one walk per pixel only gains);
  // the megakernel where the geometry's calibration found the launch throughput-bound (OrderSlot::masks_pay).
  // A launch without a measured order (too small, calibrating, tile order off) takes none.  2: every launch.
  const bool want = f.tile_masks == 2 || (f.tile_masks == 1 && (prim || (ordered && f.masks_pay)));
  p.masks = want && f.masks_ok && p.kind >= 0 && !deferred && p.mode == RT_MODE_REFL && !f.family && f.n_objects <= 32;
  // (a deferred slot's entries carry split parts: no plain tiles to gather)
  p.records = p.masks && f.tile_records && !(ordered && f.slot_deferred);
  // (a calibrating kernel renders every tile: cost[tile] is a tile's full time)
  p.sky = p.records && !calibrate && f.sky_fill && f.sky_ok;
  // Lean tiles: a megakernel launch of the masked program that reads records and does not calibrate (the
  // calibrating and the primary-ray kernels hold no exit for the bit, so their tables never carry it; a deferred
  // or mask-free launch reads no records at all).
  p.lean = f.lean_tiles && f.has_lean && p.path == LaunchPlan::MEGA && p.kind == SPEC_ROWS && p.records && !calibrate;
  // Traced tile masks: a traced table costs its pass, the counts and a second gather once (4K globes: 142 + 56 +
  // 19 us, four fifths of the 178 us frame) and gains per launch (33 us there), so it is repaid after seven
  // launches.  RT_OPT_TRACED_MASKS 1 takes it only where RT_OPT_TILE_MASKS 1 itself would pick the masked megakernel
  // -- a measured order whose calibration found the launch throughput-bound -- and only once the upload has been
  // rendered RT_TRACED_MIN_LAUNCHES times (the break-even: a host that stops there has paid at most twice the
  // cheaper choice; a host that uploads every frame, the reference's GUI, never pays); until then the launch reads
  // the predicate's table.  2 and 3: every megakernel launch that takes records.  The words hold for the megakernel's
  // pixels; the calibrating kernel renders every tile and the primary-ray kernel keeps the predicate's words.
  // The table's form: 1 and 3 take the one whose entries with a pixel on a boxed object are traced as well (their
  // shadow and refl words, and the flag that lets trace() read them); 2 keeps the floor-only form, whose object
  // entries hold the predicate's words and no flag -- the same-library A/B partner of 3.
  const bool want_traced = f.traced_masks == 2 || f.traced_masks == 3 || (f.traced_masks == 1 && ordered && f.masks_pay &&
                                                   f.launches_since_upload >= RT_TRACED_MIN_LAUNCHES);
  p.traced = want_traced && f.has_check && p.path == LaunchPlan::MEGA && p.kind == SPEC_ROWS && p.records && !calibrate;
  p.traced_objects = p.traced && f.traced_masks != 2;
  // a megakernel launch without a table runs the program's mask-free megakernel (SPEC_ROWS_NOMASK)
  if (p.kind == SPEC_ROWS && !p.masks && f.has[SPEC_ROWS_NOMASK]) p.kind = SPEC_ROWS_NOMASK;
  // With the scene-specialised megakernel loaded for these launches its costliest tiles finish so
  // much sooner that the deferred kernel no longer pays anywhere: lone 4K rank shares at N = 4 / 8
  // (tail ratios 1.6 / 3.0) 0.109 / 0.098 ms against 0.156 / 0.117 ms deferred, 1080p d5 (ratio 1.6)
  // 0.104 against 0.136 ms (profiles/r06d_kernel_choice.txt): the tail-bound choice is for the
  // generic kernels only.
  const bool spec_mega = f.loaded && f.mode == RT_MODE_REFL && f.has_rows_ordered && p.fc == f.fc;
  p.defer_forced = eligible && dmode == 1;
  p.defer_if_tail = auto_ok && dmode == -1 && f.n_tiles < RT_DEFERRED_MAX_TILES && !spec_mega;
  return p;
}

// ---- order_from_costs ---------------------------------------------------------------------------------
struct OrderParams {
  double slots;                   // wave slots of the calibrated kernel: CUs x 4 SIMDs x its waves per SIMD
  bool defer_forced, defer_if_tail;   // LaunchPlan's; both false: a plain longest-first permutation (launch_views)
  int split_max_log2;             // RT_SPLIT_MAX_LOG2
  bool xcd;                       // a non-deferred order goes by 128-byte line and XCD (xcd_line_order)
  int tiles_x, line_tiles;        //   its geometry: tiles per row, tiles per 128-byte line
};
struct TileOrder {
  std::vector<int32_t> entries;   // the tiles, or tile | part << 20 | log2 parts << 24 in a deferred order
  bool deferred, masks_pay;
};

// Primary-ray launches (max_depth 0: one intersection and its shading per pixel, so the frame's
// stores are a large share of the kernel) take an XCD-aware tile order.  The RGBA8 frame's 128-byte
// lines each hold one row of `group` horizontally adjacent 8x8 tiles; cost-sorted, those tiles run at
// different times on different XCDs (workgroups are dealt to the 8 XCDs round-robin: entries e and
// e + 8 share one).  The XCD-aware order keeps the cost sort at the granularity of a line's tiles
// (their costliest first) and places one line's tiles at entries e, e + 8, e + 16, ... of a block of
// 8 x group entries: one XCD renders them back to back.  Measured on every launch
// (profiles/r07n_xcd_order_ab.txt): the sphere 1080p d0 -3 %, globes 1080p d5 -1.2 %, 4K -0.2 %, but
// anim120 1.6 % slower and the partial-line writes do not merge (4K WRITE_SIZE +36 MiB); with plain
// stores as well the sphere gains 9 % but a store-policy branch costs the deeper launches up to 3 %
// (profiles/r08o_xcdp_ab.txt, r08q_cached_ab.txt) -- so the order alone, for max_depth 0 only.
inline void xcd_line_order(std::vector<int32_t>& order, const std::vector<uint32_t>& cost, int tiles_x, int group) {
  const size_t n = order.size(), nq = n / (size_t)group, qx = (size_t)(tiles_x / group);
  std::vector<uint32_t> qcost(nq, 0);
  for (size_t t = 0; t < n; ++t) {
    const size_t q = (t / (size_t)tiles_x) * qx + (t % (size_t)tiles_x) / (size_t)group;
    qcost[q] = std::max(qcost[q], cost[t]);
  }
  std::vector<int32_t> qorder(nq);
  for (size_t q = 0; q < nq; ++q) qorder[q] = (int32_t)q;
  std::stable_sort(qorder.begin(), qorder.end(), [&](int32_t x, int32_t y) { return qcost[x] > qcost[y]; });
  size_t e = 0;
  for (size_t g = 0; g < nq; g += 8) {
    const size_t m = std::min<size_t>(8, nq - g);
    for (int j = 0; j < group; ++j)
      for (size_t i = 0; i < m; ++i) {
        const size_t q = (size_t)qorder[g + i];
        order[e++] = (int32_t)((q / qx) * (size_t)tiles_x + (q % qx) * (size_t)group + (size_t)j);
      }
  }
}

inline TileOrder order_from_costs(const std::vector<uint32_t>& cost, const OrderParams& p) {
  const size_t n_tiles = cost.size();
  TileOrder o;
  // Longest-first: every tile placed by its own measured cost (runs of 2-30 neighbouring tiles
  // sorted together, zigzag and partly row-major orders measured 3-60 % slower,
  // profiles/r01ah_tile_order_sweep.txt, r02k_order_ab.txt).
  o.entries.resize(n_tiles);
  for (size_t i = 0; i < n_tiles; ++i) o.entries[i] = (int32_t)i;
  std::stable_sort(o.entries.begin(), o.entries.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
  // The tail measure: costliest tile against the work per wave slot.  It decides two things.
  // Tile masks (RT_OPT_TILE_MASKS 1): the masked megakernel removes work from the tiles whose walks are
  // provably empty (floor, sky) and costs every walk of every tile a few percent.  A launch that fills the
  // GPU many times over gains the difference (4K globes: -2.8 %); one whose time is set by its costliest
  // tiles -- deep reflection chains, whose walks beyond depth 1 take no mask -- only pays (1080p globes
  // d5: +1.4 %).  And the deferred kernel (RT_DEFERRED_MAX_TILES), where the plan leaves it to the tail.
  uint64_t sum = 0, mx = 0;
  for (uint32_t v : cost) { sum += v; mx = v > mx ? v : mx; }
  const bool tail = (double)mx > (double)sum / p.slots;
  o.masks_pay = !tail;
  o.deferred = p.defer_forced || (p.defer_if_tail && tail);
  if (o.deferred) {
    // Split the costliest tiles over P = 2, 4 or 8 waves (cost >= k * P * the median tile):
    // their shadow rays then spread over P x 64 lanes.  The factor k: 1 below 24000 tiles, 1.5
    // above.  Swept at 1 / 1.25 / 1.5 / 2 / 3
    // (profiles/r02bo_split_sweep.txt): the 4K N = 8 share (16320 tiles) 0.150 / 0.152 / 0.172 /
    // 0.170 / 0.183 ms; the N = 4 share (32400 tiles) 0.209 / 0.192 / 0.190 / 0.200 / 0.232 ms;
    // the whole 1080p d5 frame (32400 tiles) 0.208 / 0.189 / 0.184 / 0.181 / 0.225 ms.
    const double split_k = n_tiles < 24000 ? 1.0 : 1.5;
    std::vector<uint32_t> sorted_cost(cost);
    std::nth_element(sorted_cost.begin(), sorted_cost.begin() + n_tiles / 2, sorted_cost.end());
    const double med = std::max(1.0, (double)sorted_cost[n_tiles / 2]);
    std::vector<int32_t> split;
    split.reserve(n_tiles + n_tiles / 8);
    for (size_t i = 0; i < n_tiles; ++i) {
      const uint32_t t = (uint32_t)o.entries[i];
      int lp = 0;
      while (lp < p.split_max_log2 && cost[t] >= split_k * med * (double)(2 << lp)) ++lp;
      for (int part = 0; part < (1 << lp); ++part)
        split.push_back((int32_t)(t | ((uint32_t)part << 20) | ((uint32_t)lp << 24)));
    }
    o.entries.swap(split);
  } else if (p.xcd) {
    xcd_line_order(o.entries, cost, p.tiles_x, p.line_tiles);
  }
  return o;
}

}  // namespace rt
