// wf_plan.h -- the wavefront path's launch as pure host code, as launch_plan.h is the row launches': plain C++17, no
// HIP header and no rt_device.h, so tests/test_wf_plan.py compiles and runs it on a CPU.  The counter block's names
// (WfCount, WfPairCount), the level tables (wf_level_offset), the three layouts, the pair lists' size (wf_list_size),
// plan_wavefront and the fold schedule; k_wavefront.hip and k_wf_pairs.hip carry a plan out.
#pragma once
#include "launch_plan.h"   // rt_blob.h's RT_MAX_DEPTH_CAP and RtTravC
#include "wf_sort.h"       // the bucket sort's bin limits

#ifndef RT_WF_FOLD_SPAN
#define RT_WF_FOLD_SPAN 3                // levels folded per launch (1..3)
#endif
static_assert(RT_WF_FOLD_SPAN >= 1 && RT_WF_FOLD_SPAN <= 3, "fold span");
#ifndef RT_WFP_CAND_COUNTS
#define RT_WFP_CAND_COUNTS 1             // the candidate kernels count their pairs for the sorts
#endif

namespace rt {
// The rows of a launch as the kernels receive them (BandGeometry's four, as ints: 16 bytes of kernel arguments).
struct WfRows { int y_first, band_rows, band_pitch, n_rows; };

// ---- the counter block: 64 words (256 bytes), zeroed when a launch starts ------------------------------
// The level kernels address it as WfArena::count, the pair kernels its pair block as WfPairs::count.
constexpr int RT_WF_COUNT_WORDS = 64, RT_WFP_LOG_LEVELS = 12;
enum WfCount : int {
  WFC_LEVEL = 0,                        // [WFC_LEVEL + d], d = 0 .. RT_MAX_DEPTH_CAP + 1: rays appended to level d (d >= 1)
  WFC_OVERFLOW = RT_MAX_DEPTH_CAP + 2,  // a ray found its level full (wf_fixup_kernel re-renders its pixel)
  WFC_PAIRS = 32,                       // the pair block: WfPairs::count
};
enum WfPairCount : int {
  WFP_NEAREST = 0, WFP_SHADOW = 1,      // pairs the level's nearest / shadow pass emitted (may exceed the lists' capacity)
  WFP_WRAPPED = 2,                      // one of the two passed 2^31
  WFP_NEED = 3, WFP_WRAP = 4,           // sticky over the launch: the most pairs a level emitted beyond the capacity; any wrap
  WFP_LOG = 5,                          // [wfp_log(d, shadow)], d <= RT_WFP_LOG_LEVELS: level d's two counts (diagnostics)
};
constexpr int wfp_log(int d, bool shadow) { return WFP_LOG + 2 * d + (shadow ? 1 : 0); }
static_assert(WFC_OVERFLOW < WFC_PAIRS, "wavefront counter block");
static_assert(WFC_PAIRS + wfp_log(RT_WFP_LOG_LEVELS, true) < RT_WF_COUNT_WORDS, "wavefront counter block: 256 bytes");

// ---- the level tables ---------------------------------------------------------------------------------
// A level's table: one array of `len` entries per field (len: the pixel slots for level 0, cap for levels >= 1), the
// doubles first, in this order.  Level 0's rays are the camera's and nothing sorts them: its table holds the doubles
// from WF_F64_0 on and the words WF_I32_0 .. WF_I32_0_END - 1 only.
enum WfF64 : int { WF_OX, WF_OY, WF_OZ, WF_DX, WF_DY, WF_DZ, WF_LR, WF_LG, WF_LB, WF_WT, WF_WR, WF_N_F64, WF_F64_0 = WF_LR };
enum WfI32 : int { WF_PIX, WF_CT, WF_CR, WF_KEY, WF_VAL, WF_PAR, WF_N_I32, WF_I32_0 = WF_CT, WF_I32_0_END = WF_KEY };
constexpr size_t RT_WF_BYTES0 = (WF_N_F64 - WF_F64_0) * 8 + (WF_I32_0_END - WF_I32_0) * 4, RT_WF_BYTES = WF_N_F64 * 8 + WF_N_I32 * 4;
constexpr size_t wf_level_offset(size_t slots, size_t cap, int d) {
  return d == 0 ? 0 : slots * RT_WF_BYTES0 + (size_t)(d - 1) * cap * RT_WF_BYTES;
}

// ---- the three layouts: byte offsets into one allocation each, and its size -----------------------------
constexpr size_t wf_al(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr uint32_t RT_WF_LEVEL_BINS = 4096;                 // bucket-sort bins of a non-pair level (the key's top 12 bits)
constexpr uint32_t RT_WFP_BIN_WORDS = RT_BS_MAX_BINS;       // one bucket sort's scratch (wf_sort.hip: counts + run cursors)
static_assert(RT_WF_LEVEL_BINS <= RT_BS_MAX_BINS, "level sort bins");
// The level arena: the level tables at 0, the counter block, a flag per pixel slot, the sorted keys and the key
// order of the level being traced (cap words each), the level sort's scratch.
struct WfArenaLayout { size_t count, ovf, kout, perm, tmp, bytes; };
inline WfArenaLayout wf_arena_layout(size_t slots, size_t cap, int max_depth) {
  WfArenaLayout a;
  a.count = wf_al(wf_level_offset(slots, cap, max_depth + 1));
  a.ovf = a.count + RT_WF_COUNT_WORDS * 4;
  a.kout = wf_al(a.ovf + slots);
  a.perm = a.kout + cap * 4;
  a.tmp = wf_al(a.perm + cap * 4);
  a.bytes = a.tmp + RT_WF_LEVEL_BINS * 4 + 256;
  return a;
}
// The pair path's arrays per ray of a level (R: the larger of the pixel slots and the level capacity): R u64 (the
// nearest distance's bits), R i32 (the nearest object), 3 x R doubles (the hit point), R x lights words twice (a shadow
// ray's hit count, its opaque flag), 4 x R words (the hit-point keys and slots, as written and as sorted).
struct WfRayLayout { size_t tmin, omin, px, kcnt, opq, hkey, bytes; };
inline WfRayLayout wf_ray_layout(size_t R, int n_lights) {
  const size_t nl = (size_t)std::max(1, n_lights);
  WfRayLayout r;
  r.tmin = 0;
  r.omin = wf_al(R * 8);
  r.px = wf_al(r.omin + R * 4);
  r.kcnt = wf_al(r.px + 3 * R * 8);
  r.opq = wf_al(r.kcnt + R * nl * 4);
  r.hkey = wf_al(r.opq + R * nl * 4);
  r.bytes = wf_al(r.hkey + 4 * R * 4);
  return r;
}
// The pair lists for `cap` pairs (a multiple of 64): the three sorts' scratch (nearest, hit points, shadow), 4 x cap
// words (the pairs as emitted and as sorted: object, ray id), cap doubles (the sorted pair's distance).
struct WfListLayout { size_t bins, key, tp, bytes; };
inline WfListLayout wf_list_layout(size_t cap) {
  WfListLayout l;
  l.bins = 0;
  l.key = 3 * RT_WFP_BIN_WORDS * 4;
  l.tp = l.key + 4 * cap * 4;
  l.bytes = wf_al(l.tp + cap * 8);
  return l;
}

// ---- the pair lists' size -----------------------------------------------------------------------------
// The lists hold `have` pairs (0: none yet) and a level of `lcap` rays needs `need` (0: whatever there is).  First
// size: 4 pairs per ray of a full level (fractal.scene needs ~3); a level that emitted more grows them to a quarter
// beyond what it needed (RT_OPT_WAVEFRONT_CAP 1 % makes the first size tiny: the overflow tests take that path).
// The pair ids are 31-bit: 0x7fffffc0 pairs at most.
struct WfListSize { bool grow, refused; size_t cap; char error[80]; };
inline WfListSize wf_list_size(size_t have, size_t lcap, size_t need) {
  WfListSize s = {};
  s.cap = have;
  if (have && need <= have) return s;
  s.grow = true;
  s.cap = std::min<size_t>(0x7fffffc0ull, std::max<size_t>(need + need / 4, 4 * lcap) + 63) & ~(size_t)63;
  s.refused = need > s.cap;
  if (s.refused) snprintf(s.error, sizeof s.error, "wavefront pair list of %zu pairs too large", need);
  return s;
}

// ---- plan_wavefront -----------------------------------------------------------------------------------
constexpr uint32_t RT_WFP_LDS_TRAV_MAX = 1280;    // nodes (40 KB of RtTravC) staged in LDS at most; larger: global loads
struct WfFacts {
  size_t n_tiles;                 // the launch
  int max_depth;
  bool f64;
  int cap_pct, pairs_opt;         // RT_OPT_WAVEFRONT_CAP, RT_OPT_WAVEFRONT_PAIRS 0 / 1 / 2
  bool fast_clamp;
  int shadow_pow, n_objects, n_lights, n_trav;   // the uploaded scene (RtDevScene)
  bool any_transparent, colour_fast;
  bool global_trav;               // a diagnostic build's RT_WFP_GLOBAL_TRAV: no hierarchy in LDS
};
struct WfPlan {
  bool refused;
  char error[80];                 // refused: the message (RT_ERR_UNSUPPORTED)
  size_t slots, cap, rays;        // level 0 = the pixel slots (8x8 tiles x 64), levels >= 1: cap rays each; rays: the larger
  int max_depth;
  bool refr, fc, f64;             // the kernels' template flags
  int first_pair_level;           // levels from this one on take the pair path; -1: none
  bool pairs_level(int d) const { return first_pair_level >= 0 && d >= first_pair_level; }
  bool lds_trav;                  // the candidate walks read the hierarchy from LDS (4-wave workgroups)
  bool counted;                   // the candidate kernels count their pairs by object for the sorts
  size_t trav_lds, hist_lds;      //   their dynamic LDS: the staged hierarchy, the histogram
  int cbits;                      // hit-point key: the object above this many bits of the hit point's cell
  WfArenaLayout arena;
  WfRayLayout ray;
};
inline WfPlan plan_wavefront(const WfFacts& f) {
  WfPlan p = {};
  p.slots = f.n_tiles * 64;
  // levels >= 1: RT_OPT_WAVEFRONT_CAP % of the pixel slots, in whole waves, one at least
  p.cap = std::max<size_t>(64, (p.slots * (size_t)f.cap_pct / 100 + 63) & ~(size_t)63);
  p.rays = std::max(p.slots, p.cap);
  p.refused = p.cap > 0x7fffffffull || p.slots > 0x7fffffffull;
  if (p.refused) snprintf(p.error, sizeof p.error, "wavefront launch of %zu pixel slots too large", p.slots);
  if (p.refused) return p;
  p.max_depth = f.max_depth;
  p.refr = f.any_transparent;
  p.fc = f.colour_fast && f.fast_clamp;
  p.f64 = f.f64;
  // The pair path needs an order-free shadow product (shadow_pow), an object per sort bin, and 32-bit shadow-ray ids
  // (slot * n_lights + light): launches whose ids would not fit keep the wave walk (the pair counts are checked
  // against 2^31 on the device, wfp_cand_kernel).
  const bool pairs = f.pairs_opt > 0 && f.shadow_pow != 0 && f.n_objects > 0 && f.n_objects < (int)RT_BS_MAX_BINS &&
                     (uint64_t)p.rays * (uint64_t)std::max(1, f.n_lights) < (1ull << 32);
  p.first_pair_level = !pairs ? -1 : f.pairs_opt == 2 ? 0 : 1;
  const uint32_t nobj = (uint32_t)f.n_objects;
  p.lds_trav = (uint32_t)f.n_trav <= RT_WFP_LDS_TRAV_MAX && !f.global_trav;
  p.counted = nobj <= RT_WFP_BIN_WORDS / 2 && RT_WFP_CAND_COUNTS;   // the fused-scan sorts: <= 2048 objects
  p.trav_lds = p.lds_trav ? (size_t)f.n_trav * sizeof(RtTravC) : 0;
  p.hist_lds = p.counted ? (size_t)nobj * 4 : 0;
  // the hit points' order: at most 2048 buckets of (hit object, coarse hit-point cell): the fused-scan sort's bins
  while (p.cbits < 12 && ((nobj + 1u) << (p.cbits + 1)) <= RT_WFP_BIN_WORDS / 2) ++p.cbits;
  p.arena = wf_arena_layout(p.slots, p.cap, f.max_depth);
  p.ray = wf_ray_layout(p.rays, f.n_lights);
  return p;
}

// ---- the fold schedule --------------------------------------------------------------------------------
// After the last traced level: the folds, deepest first, RT_WF_FOLD_SPAN levels per launch (levels d .. d + span - 1).
// The deepest level's rays have no children (their colour is their hit record) unless it is level 0, whose fold
// writes the pixels: the last step always starts at level 0.
struct WfFolds { int n; struct Step { int d, span; } step[RT_MAX_DEPTH_CAP + 2]; };
inline WfFolds wf_fold_schedule(int last) {
  WfFolds s = {};
  for (int top = last > 0 ? last - 1 : 0; top >= 0; top = s.step[s.n - 1].d - 1) {
    const int d = std::max(0, top - RT_WF_FOLD_SPAN + 1);
    s.step[s.n++] = {d, top - d + 1};
  }
  return s;
}
}  // namespace rt
