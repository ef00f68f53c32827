// k_rows.hip -- the row kernels (one thread per pixel, one wave per 8x8 tile) and their launches:
// rt_render_rows / _f64 / _row_bands / _row_bands_rgb8 (include/rt_abi.h), i.e. the reference's row
// loop DebugWindow::render_lines (raydebugger/debug_window.rs:74-87) over get_pixel
// (raytracer/raytracer.rs:359-363).  The per-ray code is rt_device.h's; which kernel a launch runs and
// what it is handed is launch_plan.h's (plan_row_launch), launch_bands carries the plan out.
#include <stdio.h>

#include "rt_device.h"
#include "rt_ctx.h"
#include <hip/hip_ext.h>

namespace {

// The megakernel: trace() per lane (rt_device.h rows_body).  Waves per SIMD per mode: see
// RT_WAVES_MODE.  The first frames of the per-lane stack live in LDS.
template <int MODE, bool F64, bool CAL = false, bool FC = false>
__global__ __launch_bounds__(RT_WG_THREADS) __attribute__((amdgpu_waves_per_eu(RT_WAVES_MODE(MODE)))) void
render_rows_kernel(RtDevScene S, int y_first, int band_rows, int band_pitch, int n_rows, int max_depth,
                   uint8_t* __restrict__ out, size_t stride, const int32_t* __restrict__ order,
                   uint32_t* __restrict__ cost, int rgb) {
  __shared__ double s_frames[rows_lds_doubles<MODE>()];   // frame stack, see trace()
  rows_body<MODE, F64, CAL, FC>(S, y_first, band_rows, band_pitch, n_rows, max_depth, out, stride, order, cost, rgb,
                                (lds_f64*)s_frames);
}

// The deferred-shadow kernel (rt_device.h deferred_body), for launches of few tiles (a multi-GPU
// rank's share) whose time is set by their costliest tiles.  A kernel of its own: the megakernel path
// and this one in ONE kernel measured 3.4x slower than either (profiles/r02g_ab.txt: both paths' code
// hot on one CU at once).
template <bool F64, bool CAL = false, bool FC = false, bool REFR = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU_DEFERRED))) void
render_rows_deferred_kernel(RtDevScene S, int y_first, int band_rows, int band_pitch, int n_rows, int max_depth,
                            uint8_t* __restrict__ out, size_t stride, const int32_t* __restrict__ order,
                            uint32_t* __restrict__ cost, int rgb) {
  __shared__ ShadowWin win;
  deferred_body<F64, CAL, FC, REFR>(S, y_first, band_rows, band_pitch, n_rows, max_depth, out, stride, order, cost, rgb,
                                    &win);
}

}  // namespace

using namespace rt;

// plan_row_launch's inputs as the context holds them, with rt_device.h's constants
LaunchFacts rt::launch_facts(const rt_ctx* c, int max_depth, bool f64, size_t n_tiles, const rt_ctx::OrderSlot* slot,
                             bool calibrate) {
  LaunchFacts f = {};
  f.any_transparent = c->dev.any_transparent != 0; f.ray_chains = c->dev.ray_chains != 0; f.colour_fast = c->dev.colour_fast != 0;
  f.n_lights = c->dev.n_lights; f.n_objects = c->dev.n_objects; f.views = c->views.kind != 0;
  f.kernel_opt = c->kernel_opt; f.tile_order = c->tile_order; f.tile_masks = c->tile_masks;
  f.tile_records = c->tile_records; f.sky_fill = c->sky_fill; f.fast_clamp = c->fast_clamp;
  f.sky_ok = c->sky_ok; f.masks_ok = masks_usable(c);
  f.max_depth = max_depth; f.f64 = f64; f.n_tiles = n_tiles;
  f.slot = !slot ? LaunchFacts::NONE : calibrate ? LaunchFacts::CALIBRATING : LaunchFacts::ORDERED;
  if (slot) { f.slot_deferred = slot->deferred; f.masks_pay = slot->masks_pay; f.wf_tune = slot->wf_tune; }
  const SpecProgram& sp = c->spec.prog;
  f.loaded = c->spec.loaded; f.mode = sp.mode; f.fc = sp.fc; f.family = sp.family != 0; f.two_eyes = sp.two_eyes;
  for (int k = 0; k < SPEC_KINDS; ++k) f.has[k] = spec_fn(c, k, f64, calibrate) != nullptr;
  f.has_rows_ordered = spec_fn(c, SPEC_ROWS, f64, false) != nullptr;
  f.sh_trcap = RT_SH_TRCAP; f.split_tile_mask = RT_SPLIT_TILE_MASK;
  f.refl_pooled = RT_LDS_POOL_REFL > 0; f.pool_byte_index = RT_POOL_OBJ_INDEX != 0;
  f.lean_tiles = c->lean_tiles;
  f.has_lean = spec_fn(c, SPEC_LEAN, f64, false) != nullptr && spec_fn(c, SPEC_LEAN_CHECK, false, false) != nullptr;
  f.traced_masks = c->traced_masks;
  f.has_check = spec_fn(c, SPEC_LEAN_CHECK, false, false) != nullptr;
  f.launches_since_upload = c->launches_since_upload;
  return f;
}

static int launch_bands(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                        int32_t max_depth, void* out, size_t stride, void* stream, bool f64, bool rgb = false) {
  if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  const BandGeometry g = band_geometry(c->dev.width, c->dev.height, y_first, band_rows, band_pitch, n_bands);
  if (g.status == BandGeometry::NOTHING) return RT_OK;
  if (g.status != BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  const size_t row_bytes = (size_t)c->dev.width * (f64 ? 32 : rgb ? 3 : 4), n_tiles = g.n_tiles;
  const int rgbi = rgb && !f64 ? 1 : 0;
  if (stride < row_bytes) return fail(RT_ERR_INVALID, "row stride %zu < %zu", stride, row_bytes);
  if (max_depth < 0) max_depth = c->max_depth;
  if (max_depth > RT_MAX_DEPTH_CAP) return fail(RT_ERR_UNSUPPORTED, "max_depth %d > %d", max_depth, RT_MAX_DEPTH_CAP);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  (void)spec_poll(c);                     // the scene-specialised kernels, once their background compile is done
  c->last_masked = false;
  c->last_records = false;
  c->last_traced = false;
  c->last_rec_slot = nullptr;
  c->last_lean_slot = nullptr;
  // a host buffer: render into the context's scratch, copy back at the end (finish_launch)
  uint8_t* target = (uint8_t*)out;
  size_t tstride = stride;
  if (!is_device_ptr(out)) {
    RT_TRY(ensure_scratch(c, row_bytes * g.n_rows));
    target = (uint8_t*)c->scratch;
    tstride = row_bytes;
  }
  const HostCopy hc = {target == out ? nullptr : out, stride, target, tstride, row_bytes, g.n_rows};
  const int a0 = (int)y_first, a1 = (int)band_rows, a2 = (int)band_pitch, a3 = (int)g.n_rows;
  const WfRows wf_rows = {(int)g.y_first, (int)g.band_rows, (int)g.band_pitch, (int)g.n_rows};
  // a two-eye scene (stereoscopic, anaglyph): one launch of the view megakernel over both eyes' tiles
  if (c->views.kind) return launch_views(c, st, a0, a1, a2, a3, max_depth, target, tstride, f64, rgbi, hc);
  const int32_t key[8] = {a0, a1, a2, a3, max_depth, f64 ? 1 : 0, c->dev.width, RT_CAMERA_PERSPECTIVE};
  rt_ctx::OrderSlot* slot = nullptr;
  bool calibrate = false;
  if (c->kernel_opt != RT_KERNEL_WAVEFRONT) RT_TRY(acquire_order(c, key, n_tiles, st, &slot, &calibrate));   // (it takes no order)
  const LaunchPlan plan = plan_row_launch(launch_facts(c, max_depth, f64, n_tiles, slot, calibrate));
  if (c->launches_since_upload < 0xffffffffu) ++c->launches_since_upload;
  const int32_t* order = slot && !calibrate ? slot->d_order : nullptr;
  uint32_t* cost = calibrate ? slot->d_cost : nullptr;
  const dim3 grid(order ? slot->grid : (unsigned)n_tiles);
  c->last_kernel = plan.last_kernel;
  if (plan.refused)
    return fail(RT_ERR_UNSUPPORTED, "a pooled kernel for a scene of %d objects (one-byte object index)", c->dev.n_objects);
  // A mask table that is new since the upload is filled here, and the launch's dispatch records gathered,
  // AHEAD of the timing event: rt_ctx_last_kernel_ms reports the render kernel alone.
  rt_ctx::MaskSlot* ms = nullptr;
  const RtTileRec* recs = nullptr;
  const void* rec_slot = nullptr;
  if (plan.masks) RT_TRY(mask_slot(c, st, a0, a1, a2, a3, n_tiles, &ms));
  if (plan.records) RT_TRY(launch_records(c, st, ms, order, order ? slot->order_id : 0, grid.x, plan.lean,
                                        plan.traced ? (plan.traced_objects ? 2 : 1) : 0, &recs,
                                        &rec_slot));
  const uint32_t* masks = ms ? ms->d_masks : nullptr;
  c->last_masked = plan.masks;
  c->last_records = plan.records;
  c->last_traced = plan.traced;
  c->last_rec_slot = rec_slot;
  c->last_rec_id = record_id(rec_slot);
  if (c->timing) RT_HIP(hipEventRecord(c->ev0, st));
  if (plan.path == LaunchPlan::WAVEFRONT) {
    RT_TRY(launch_wavefront(c, st, wf_rows, max_depth, target, tstride, f64, rgbi, n_tiles));
    return finish_launch(c, st, hc, true);
  }
  c->last_sky_slot = plan.sky ? rec_slot : nullptr;
  c->last_sky_id = plan.sky ? record_id(rec_slot) : 0;
  c->last_lean_slot = plan.lean ? rec_slot : nullptr;
  c->last_lean_id = plan.lean ? record_id(rec_slot) : 0;
  // the row kernels carry the context's completion event for this stream as their stop event
  hipEvent_t mev = nullptr;
#ifndef RT_DIAG_NO_MARKS
  RT_TRY(mark_event(c, st, &mev));
#endif
  if (plan.tune) RT_HIP(hipEventRecord(c->tev0, st));
  if (plan.kind >= 0) {
    void* kargs[] = {&c->dev, (void*)&a0, (void*)&a1, (void*)&a2, (void*)&a3, &max_depth, &target, &tstride,
                     (void*)&order, &cost, (void*)&rgbi, (void*)&masks, (void*)&recs};   // (a kernel reads as
    // many as it declares: the masked single-scene kernels take the records, spec_text.cpp)
    // hipExtModuleLaunchKernel takes the global work size in work-items (grid x 64)
    // the lean kernel first, over the same entries and operands: it renders the entries whose record says lean,
    // the megakernel's waves of those return at entry (inside the frame's timing pair; the completion event stays
    // the megakernel's)
    // Its grid: the lean entries are the cheap end of the cost order, one run of entries holds them all; once the
    // table's check has completed the host knows that run (a pinned word, never a wait) and the kernel is launched
    // over it alone -- the table's address moved to the run's first record, the kernel unchanged.  Until then:
    // every entry, the others' waves return at once.
    if (plan.lean) {
      uint32_t first = 0, end = grid.x;
      (void)record_lean_range(rec_slot, &first, &end);
      const RtTileRec* lean_recs = recs + first;
      void* largs[] = {&c->dev, (void*)&a0, (void*)&a1, (void*)&a2, (void*)&a3, &max_depth, &target, &tstride,
                       (void*)&order, &cost, (void*)&rgbi, (void*)&masks, (void*)&lean_recs};
      if (end > first)
        RT_HIP(hipExtModuleLaunchKernel(spec_fn(c, SPEC_LEAN, f64, false), (end - first) * 64u, 1, 1, 64, 1, 1, 0, st, largs,
                                        nullptr, nullptr, nullptr, 0));
    }
    RT_HIP(hipExtModuleLaunchKernel(spec_fn(c, plan.kind, f64, calibrate), grid.x * 64u, 1, 1, 64, 1, 1, 0, st, kargs,
                                    nullptr, nullptr, mev, 0));
  } else {
    with_flags(f64, calibrate, plan.fc, [&](auto F, auto C, auto K) {
      if (plan.path == LaunchPlan::DEFERRED)
        with_bool(plan.chain, [&](auto R) {
          hipExtLaunchKernelGGL(
              (render_rows_deferred_kernel<decltype(F)::value, decltype(C)::value, decltype(K)::value, decltype(R)::value>),
              grid, dim3(64), 0, st, nullptr, mev, 0, c->dev, a0, a1, a2, a3, max_depth, target, tstride, order, cost, rgbi);
        });
      else
        with_mode(plan.mode, [&](auto M) {
          hipExtLaunchKernelGGL((render_rows_kernel<decltype(M)::value, decltype(F)::value, decltype(C)::value, decltype(K)::value>),
                                grid, dim3(RT_WG_THREADS), 0, st, nullptr, mev, 0, c->dev, a0, a1, a2, a3, max_depth, target,
                                tstride, order, cost, rgbi);
        });
    });
  }
  RT_HIP(hipGetLastError());
  if (plan.tune) RT_HIP(hipEventRecord(c->tev1, st));
  RT_TRY(finish_launch(c, st, hc, false));
  if (plan.tune) {                    // synchronous, once per ray-tree geometry (plan_row_launch)
    float mega_ms = 0.0f, wf_ms = 0.0f;
    RT_HIP(hipEventSynchronize(c->tev1));
    RT_HIP(hipEventElapsedTime(&mega_ms, c->tev0, c->tev1));
    // one untimed wavefront launch first: it allocates (or grows) the wavefront and pair arenas, which
    // the megakernel's timed launch had no counterpart of (a cold first launch could otherwise decide
    // the choice for the geometry)
    RT_TRY(launch_wavefront(c, st, wf_rows, max_depth, target, tstride, f64, rgbi, n_tiles));
    RT_HIP(hipEventRecord(c->tev0, st));
    RT_TRY(launch_wavefront(c, st, wf_rows, max_depth, target, tstride, f64, rgbi, n_tiles));
    RT_HIP(hipEventRecord(c->tev1, st));
    RT_HIP(hipEventSynchronize(c->tev1));
    RT_HIP(hipEventElapsedTime(&wf_ms, c->tev0, c->tev1));
    slot->wf_tune = wf_ms < mega_ms ? 2 : 1;
    static const bool order_debug = diag_env("RT_TILE_ORDER_DEBUG");
    if (order_debug)
      fprintf(stderr, "ray-tree autotune: megakernel %.3f ms, wavefront %.3f ms -> %s\n", mega_ms, wf_ms,
              slot->wf_tune == 2 ? "wavefront" : "megakernel");
  }
  if (calibrate) {
    const int line_tiles = 128 / (RT_TILE_W * 4);   // the XCD line order: RGBA8 primary-ray frames of whole, aligned lines
    const bool xcd = max_depth == 0 && !f64 && !rgbi && g.tiles_x % line_tiles == 0 && tstride % 128 == 0 &&
                     ((uintptr_t)target & 127) == 0;
    RT_TRY(finish_calibration(c, st, slot, {c->n_cu * 4.0 * RT_WAVES_MODE(plan.mode), plan.defer_forced, plan.defer_if_tail,
                                            RT_SPLIT_MAX_LOG2, xcd, g.tiles_x, line_tiles}));
  }
  return RT_OK;
}

static int launch_rows(rt_ctx* c, uint32_t y0, uint32_t y1, int32_t max_depth, void* out, size_t stride,
                       void* stream, bool f64) {
  if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (y0 > y1 || y1 > (uint32_t)c->dev.height) return fail(RT_ERR_INVALID, "bad row range [%u, %u) for height %d", y0, y1, c->dev.height);
  if (y0 == y1) return RT_OK;
  return launch_bands(c, y0, y1 - y0, y1 - y0, 1, max_depth, out, stride, stream, f64);
}

extern "C" {

int rt_render_row_bands(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                        int32_t max_depth, uint8_t* rgba8, size_t row_stride_bytes, void* stream) {
  return launch_bands(c, y_first, band_rows, band_pitch, n_bands, max_depth, rgba8, row_stride_bytes, stream, false);
}

int rt_render_row_bands_rgb8(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                             int32_t max_depth, uint8_t* rgb8, size_t row_stride_bytes, void* stream) {
  return launch_bands(c, y_first, band_rows, band_pitch, n_bands, max_depth, rgb8, row_stride_bytes, stream, false, true);
}

int rt_render_rows(rt_ctx* c, uint32_t y0, uint32_t y1, int32_t max_depth, uint8_t* rgba8,
                   size_t row_stride_bytes, void* stream) {
  return launch_rows(c, y0, y1, max_depth, rgba8, row_stride_bytes, stream, false);
}

int rt_render_rows_f64(rt_ctx* c, uint32_t y0, uint32_t y1, int32_t max_depth, double* rgba,
                       size_t row_stride_bytes, void* stream) {
  return launch_rows(c, y0, y1, max_depth, rgba, row_stride_bytes, stream, true);
}

}  // extern "C"
