// k_wavefront.hip -- the wavefront path (one recursion depth per pass over a dense level of rays): launch-wide
// secondary-ray compaction for ray-tree scenes (DESIGN.md §2 "Wavefront path").  Its level kernels and its launch;
// the pair path ((ray, object) work items sorted by object) is k_wf_pairs.hip, what the two share on the device
// rt_wavefront.h, every size, layout and choice of a launch wf_plan.h.  get_ray_color's operations per ray are
// rt_device.h's; these files reorganise WHEN they run, never what they compute.
#include <stdio.h>

#include <algorithm>

#include "rt_wavefront.h"
#include "rt_ctx.h"
#include "wf_sort.h"

namespace {

// ====================================================================== wavefront path
// get_ray_color (raytracer.rs:132-287) launch-wide, one bounce level per pass: level d holds every
// ray of recursion depth d of the launch, densely, one lane per ray.  Per level:
//   wf_trace_kernel  nearest hit, shadow rays, shading, the inside / refraction / TIR / reflection
//                    decisions of trace() (the same operations in the same order); the rays a hit
//                    spawns are appended to level d + 1 (one ballot + one atomic per wave), each with a
//                    coherence key (direction octant, Morton code of its origin); the hit record (L,
//                    the two weights, the children's slots) stays at the ray's slot;
//   sort             level d + 1's slots by key (the in-tree bucket sort of (key, slot) pairs on the key's
//                    top 12 bits, wf_sort.hip): a wave of
//                    the next pass then traces rays that start close together in similar directions,
//                    so the wave-coherent traversal walks fewer objects (the megakernel's waves walk the
//                    union of what their lanes' scattered secondary rays need);
//   wf_fold_kernel   after every level is traced, from the deepest level up (RT_WF_FOLD_SPAN levels
//                    per launch): a ray's colour from its hit record and its children's colours:
//                      refraction child: comb = in_range(L.intensify(1 - t) + C_t.intensify(t)),
//                      then a reflection child: in_range(comb.intensify(1 - rp) + C_r.intensify(rp)),
//                    exactly the post-order of raytracer.rs:256-279 (trace()'s frame fold).  Level 0's
//                    fold writes the pixels.
// Lanes whose pixel's tree ended early no longer idle in its wave (the megakernel's per-lane tree
// walk keeps a wave alive for its deepest tree): every pass starts with every lane on a live ray, and
// every pass is one workgroup per 64 rays, so the hardware dispatcher balances uneven rays.  A level
// the wave walk traces is launched with its exact count, which the host reads first (one synchronisation
// per such level: this path is for heavy, incoherent launches); a pair level is device-driven
// (k_wf_pairs.hip).  Levels >= 1 hold RT_OPT_WAVEFRONT_CAP % of the pixel slots; a
// ray that finds its level full marks its pixel, and wf_fixup_kernel re-renders marked pixels with
// trace() (same bits).
template <bool REFR, bool FC>
__device__ __forceinline__ void wf_ray(const DS& S, V3 ro, V3 rd, int depth, int max_depth, Col* Lo, double* wt,
                                       double* wr, bool* ch_t, bool* ch_r, V3* po, V3* dt, V3* dr, int* hit_obj) {
  constexpr bool SHARE = REFR, OBB = !REFR;
  wf_ray_core<REFR, FC>(
      S, ro, rd, depth, max_depth,
      [&](double* t) { return *hit_obj = nearest_hit<SHARE, OBB>(S, ro, rd, t); },
      [&](int, V3 p, V3 sdir, double ll) { return shadow_transparency<SHARE, OBB>(S, p, sdir, ll); }, Lo, wt, wr, ch_t,
      ch_r, po, dt, dr);
}

// One workgroup (wave) per 64 rays of level d (n of them): level 0 = the pixel slots in tile order,
// levels >= 1 in key order (A.perm).
template <bool REFR, bool FC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU_WF))) void wf_trace_kernel(
    RtDevScene S, WfArena A, int d, uint32_t n, WfRows rows, int max_depth) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 64u + (uint32_t)lane;
  bool live = i < n;
  const WfLevel lv = wf_level(A, d);
  V3 ro = {0.0, 0.0, 0.0}, rd = {0.0, 0.0, 0.0};
  uint32_t j = i;                                            // the ray's slot in its level
  int32_t pix = (int32_t)i;
  if (d == 0) {
    int x, r, y;
    live = live && wf_pixel(S, i, rows, &x, &r, &y);
    if (live) camera_ray_px(S, x, y, &ro, &rd);                          // get_pixel(x as f64, y as f64)
  } else if (live) {
    j = A.perm ? A.perm[i] : i;
    ro = {lv.ox[j], lv.oy[j], lv.oz[j]};
    rd = {lv.dx[j], lv.dy[j], lv.dz[j]};
    pix = lv.pix[j];
  }
  Col L = {0.0, 0.0, 0.0};
  double wt = 0.0, wr = 0.0;
  bool ch_t = false, ch_r = false;
  V3 p = {0.0, 0.0, 0.0}, dt = {0.0, 0.0, 0.0}, dr = {0.0, 0.0, 0.0};
  int oi = -1;
  if (live) wf_ray<REFR, FC>(make_ds(S), ro, rd, d, max_depth, &L, &wt, &wr, &ch_t, &ch_r, &p, &dt, &dr, &oi);
  wf_append(A, lv, d, lane, live, j, pix, L, wt, wr, ch_t, ch_r, p, dt, dr, oi);
}

// The folded colour of ray i of level d: its hit record and its children's colours -- computed here
// for the SPAN - 1 levels below d (a child has one parent: nothing is computed twice), read as stored
// (already folded) at level d + SPAN.  The same operations in the same order as one fold per level.
template <int SPAN, bool FC>
__device__ __forceinline__ Col wf_fold_node(const WfArena& A, int d, uint32_t i) {
  const WfLevel lv = wf_level(A, d);
  const Col L = {lv.Lr[i], lv.Lg[i], lv.Lb[i]};
  const int32_t ct = lv.ct[i], cr = lv.cr[i];
  auto child = [&](int32_t c) -> Col {
    if constexpr (SPAN > 1) {
      return wf_fold_node<SPAN - 1, FC>(A, d + 1, (uint32_t)c);
    } else {
      const WfLevel ch = wf_level(A, d + 1);
      return Col{ch.Lr[c], ch.Lg[c], ch.Lb[c]};
    }
  };
  Col C = L;
  if (ct >= 0) {                                             // refraction, then a pending reflection
    const double t = lv.wt[i];
    C = cadd<FC>(intensify<FC>(L, 1.0 - t), intensify<FC>(child(ct), t));
  }
  if (cr >= 0) {
    const double w = lv.wr[i];
    C = cadd<FC>(intensify<FC>(C, 1.0 - w), intensify<FC>(child(cr), w));
  }
  return C;
}

// Folds SPAN levels per launch (d .. d + SPAN - 1; level d's colours stored, or level 0's written as
// pixels): one launch boundary per SPAN levels (a boundary costs ~5 us on the pair path's small levels).
// The pixels go out by plain write-back stores (store_pixel's PLAIN), here and in the fix-up.
template <int SPAN, bool F64, bool FC>
__global__ __launch_bounds__(256) void wf_fold_kernel(RtDevScene S, WfArena A, int d, uint32_t n, const uint32_t* n_dev,
                                                      WfRows rows, uint8_t* __restrict__ out, size_t stride, int rgb) {
  if (n_dev) n = min(*n_dev, A.cap);                         // a device-driven level's count
  const WfLevel lv = wf_level(A, d);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int x = 0, r = 0, y = 0;
    if (d == 0 && (!wf_pixel(S, i, rows, &x, &r, &y) || A.ovf[i])) continue;
    const Col C = wf_fold_node<SPAN, FC>(A, d, i);
    if (d > 0) {
      lv.Lr[i] = C.r; lv.Lg[i] = C.g; lv.Lb[i] = C.b;
      continue;
    }
    store_pixel<F64, /*PLAIN=*/true>(out + (size_t)r * stride, x, C, rgb);
  }
}

// Pixels whose tree overflowed a level: the per-lane megakernel trace (same bits).  Returns at once
// when no level overflowed (one uniform load).
template <bool REFR, bool F64, bool FC>
__global__ __launch_bounds__(64) void wf_fixup_kernel(RtDevScene S, WfArena A, WfRows rows, int max_depth,
                                                      uint8_t* __restrict__ out, size_t stride, int rgb) {
  if (A.count[rt::WFC_OVERFLOW] == 0) return;
  for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < A.slots; i += gridDim.x * 64) {
    int x, r, y;
    if (!A.ovf[i] || !wf_pixel(S, i, rows, &x, &r, &y)) continue;
    V3 ro, rd;
    camera_ray_px(S, x, y, &ro, &rd);
    const Col C = trace<REFR, NoRec, 0, FC>(make_ds(S), ro, rd, max_depth);
    store_pixel<F64, /*PLAIN=*/true>(out + (size_t)r * stride, x, C, rgb);
  }
}

}  // namespace

using namespace rt;

// The wavefront path (wf_*_kernel): level 0 (the pixel slots), then each level the previous one
// appended to; then the folds, deepest level first (wf_fold_schedule); then the overflow fix-up.  A level of the
// wave walk is sorted by coherence key and launched as exactly one wave per 64 rays: the host reads its count
// first (one stream synchronisation) and stops at the first empty level.  A pair level (wfp_level) is
// device-driven: its kernels read the count themselves, and so do the folds of such levels; the host reads the
// pair path's sticky words once, after the whole launch.
int rt::launch_wavefront(rt_ctx* c, hipStream_t st, WfRows rows, int max_depth, uint8_t* target, size_t tstride, bool f64,
                         int rgbi, size_t n_tiles, int retry) {
  WfFacts f = {};                       // the launch, the context's options, the uploaded scene
  f.n_tiles = n_tiles; f.max_depth = max_depth; f.f64 = f64;
  f.cap_pct = c->wf_cap_pct; f.pairs_opt = c->wf_pairs; f.fast_clamp = c->fast_clamp;
  f.shadow_pow = c->dev.shadow_pow; f.n_objects = c->dev.n_objects; f.n_lights = c->dev.n_lights; f.n_trav = c->dev.n_trav;
  f.any_transparent = c->dev.any_transparent != 0; f.colour_fast = c->dev.colour_fast != 0;
  f.global_trav = diag_env("RT_WFP_GLOBAL_TRAV");
  const WfPlan plan = plan_wavefront(f);
  if (plan.refused) return fail(RT_ERR_UNSUPPORTED, "%s", plan.error);
  RT_TRY(grow_device(c->wf, c->wf_bytes, plan.arena.bytes));
  uint8_t* base = (uint8_t*)c->wf;
  WfArena A;
  A.base = base;
  A.count = (uint32_t*)(base + plan.arena.count);
  A.ovf = base + plan.arena.ovf;
  A.perm = nullptr;
  A.slots = (uint32_t)plan.slots;
  A.cap = (uint32_t)plan.cap;
  for (int k = 0; k < 3; ++k) {
    A.klo[k] = c->wf_klo[k];
    A.kscale[k] = 512.0 / std::max(1e-9, c->wf_khi[k] - c->wf_klo[k]);
  }
  uint32_t* kout = (uint32_t*)(base + plan.arena.kout);
  uint32_t* perm = (uint32_t*)(base + plan.arena.perm);
  uint32_t* tmp = (uint32_t*)(base + plan.arena.tmp);
  RT_HIP(hipMemsetAsync(A.count, 0, RT_WF_COUNT_WORDS * 4, st));
  RT_HIP(hipMemsetAsync(A.ovf, 0, plan.slots, st));
  // n_level[d]: the level's ray count when the host knows it (level 0, and levels the wave walk traced,
  // whose count it reads); known[d] = false: a device-driven pair level (its kernels read its counter word)
  uint32_t n_level[RT_MAX_DEPTH_CAP + 2] = {0};
  bool known[RT_MAX_DEPTH_CAP + 2] = {false};
  n_level[0] = (uint32_t)plan.slots;
  known[0] = true;
  bool any_pairs = false;
  int last = 0;
  for (int d = 0; d <= max_depth; ++d) {
    uint32_t* const count_d = A.count + WFC_LEVEL + d;
    if (!known[d] && !plan.pairs_level(d)) {                 // the wave walk needs the count: read it
      uint32_t cnt = 0;
      RT_HIP(hipMemcpyAsync(&cnt, count_d, 4, hipMemcpyDeviceToHost, st));
      RT_HIP(hipStreamSynchronize(st));
      n_level[d] = std::min<uint32_t>(cnt, A.cap);
      known[d] = true;
    }
    if (known[d] && n_level[d] == 0) break;
    const uint32_t n = n_level[d];
    last = d;
    A.perm = nullptr;
    if (plan.pairs_level(d)) {
      // the pair path reads a level in slot order: its candidate walks are per lane and its evaluations
      // run in object order (a key sort measured 0.3-0.6 ms per fractal frame slower, profiles/r03o_sort_ab.txt)
      RT_TRY(wfp_level(c, st, plan, A, d, known[d] ? n : A.cap, known[d] ? nullptr : count_d, rows, !any_pairs));
      any_pairs = true;
      continue;                                              // level d + 1: device-driven
    }
    if (d > 0) {                                             // this level's slots in key order
      // the in-tree bucket sort on the key's top 12 bits (direction octant + the 8^3-cell Morton prefix);
      // only the processing order depends on it, never a value
      const WfLevel L = wf_level(A, d);                      // host-side pointer arithmetic only
      RT_HIP(rt_wf_bucket_sort(L.key, kout, L.val, perm, n, nullptr, RT_WF_LEVEL_BINS, 30 - 12, tmp, true, st));
      A.perm = perm;
    }
    with_bool(plan.refr, [&](auto R) { with_bool(plan.fc, [&](auto K) {
      hipLaunchKernelGGL((wf_trace_kernel<decltype(R)::value, decltype(K)::value>), dim3((n + 63) / 64), dim3(64), 0, st, c->dev, A,
                         d, n, rows, max_depth);
    }); });
    RT_HIP(hipGetLastError());
  }
  const WfFolds folds = wf_fold_schedule(last);
  for (int k = 0; k < folds.n; ++k) {
    const int d = folds.step[k].d;
    const uint32_t n = known[d] ? n_level[d] : A.cap;
    const uint32_t* nd = known[d] ? nullptr : A.count + WFC_LEVEL + d;
    const dim3 gf(std::max(1u, std::min<uint32_t>((n + 255) / 256, (uint32_t)c->n_cu * 8u)));
    with_span(folds.step[k].span, [&](auto SP) { with_bool(plan.f64, [&](auto F) { with_bool(plan.fc, [&](auto K) {
      hipLaunchKernelGGL((wf_fold_kernel<decltype(SP)::value, decltype(F)::value, decltype(K)::value>), gf, dim3(256), 0, st,
                         c->dev, A, d, n, nd, rows, target, tstride, rgbi);
    }); }); });
  }
  with_flags(plan.refr, plan.f64, plan.fc, [&](auto R, auto F, auto K) {
    hipLaunchKernelGGL((wf_fixup_kernel<decltype(R)::value, decltype(F)::value, decltype(K)::value>),
                       dim3((unsigned)c->n_cu * 4u), dim3(64), 0, st, c->dev, A, rows, max_depth, target, tstride, rgbi);
  });
  RT_HIP(hipGetLastError());
  if (any_pairs) {
    // the device-driven pair levels' sticky words: ONE host synchronisation per launch.  A level whose pairs
    // outgrew the lists computed wrong hits: grow them to what it needed and render the launch again (its
    // levels recomputed from the camera rays; the tests force this path)
    static_assert(WFP_WRAP == WFP_NEED + 1, "the two sticky words are read in one copy");
    uint32_t sticky[2] = {0, 0};
    RT_HIP(hipMemcpyAsync(sticky, A.count + WFC_PAIRS + WFP_NEED, sizeof sticky, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    const uint32_t need = sticky[0], wrap = sticky[1];
    static const bool wf_debug = diag_env("RT_WF_DEBUG");
    if (wf_debug) {                       // per level: rays, nearest pairs, shadow pairs
      uint32_t cb[RT_WF_COUNT_WORDS];
      RT_HIP(hipMemcpy(cb, A.count, sizeof cb, hipMemcpyDeviceToHost));
      fprintf(stderr, "wavefront levels (rays / nearest pairs / shadow pairs):");
      for (int d = 0; d <= last && d <= RT_WFP_LOG_LEVELS; ++d)
        fprintf(stderr, " %d: %u / %u / %u;", d, d == 0 ? A.slots : cb[WFC_LEVEL + d], cb[WFC_PAIRS + wfp_log(d, false)],
                cb[WFC_PAIRS + wfp_log(d, true)]);
      fprintf(stderr, "\n");
    }
    if (wrap) return fail(RT_ERR_UNSUPPORTED, "wavefront pair count passed 2^31");
    if (need) {
      if (retry > 2) return fail(RT_ERR_DEVICE, "wavefront pair lists still overflow after %d resizes", retry);
      RT_TRY(wfp_lists(c, plan, need));   // grows (synchronises)
      return launch_wavefront(c, st, rows, max_depth, target, tstride, f64, rgbi, n_tiles, retry + 1);
    }
  }
  return RT_OK;
}
