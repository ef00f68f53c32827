// k_stereo.hip -- the row kernels of two-eye scenes: StereoscopicCamera (raytracer/camera.rs:82-141: two
// eyes side by side in one frame) and AnaglyphCamera (:143-205: red from the left eye, green and blue from
// the right).  A two-eye frame is the rays of two perspective frames, so it is ONE launch over the tiles
// of two views (rt_blob.h RtViews, rt_device.h rows_views_body): one wave per (view, 8x8 tile of that
// view), the camera wave-uniform, trace() and its register budget those of the perspective megakernels,
// every output byte written once.  The perspective kernels (k_rows.hip) take no part and no new branch.
#include "rt_device.h"
#include "rt_ctx.h"
#include <hip/hip_ext.h>

namespace {

// The view megakernel: render_rows_kernel (k_rows.hip) with the views beside the scene.
template <int MODE, bool F64, bool CAL = false, bool FC = false>
__global__ __launch_bounds__(RT_WG_THREADS) __attribute__((amdgpu_waves_per_eu(RT_WAVES_MODE(MODE)))) void
render_views_kernel(RtDevScene S, RtViews VW, int y_first, int band_rows, int band_pitch, int n_rows, int max_depth,
                    uint8_t* __restrict__ out, size_t stride, const int32_t* __restrict__ order,
                    uint32_t* __restrict__ cost, int rgb) {
  __shared__ double s_frames[rows_lds_doubles<MODE>()];   // frame stack, see trace()
  rows_views_body<MODE, F64, CAL, FC>(S, VW, y_first, band_rows, band_pitch, n_rows, max_depth, out, stride, order, cost,
                                      rgb, (lds_f64*)s_frames);
}

}  // namespace

namespace rt {

// A two-eye scene's row launch.  The entries are view 0's tiles, then view 1's; the longest-first order
// and its calibration (launch_bands) run over all of them, from RT_ORDER_MIN_TILES entries.  Always the
// view megakernel of the scene's mode, generic or specialised: RT_OPT_KERNEL's deferred and wavefront
// choices and the tile masks have no two-eye form.
int launch_views(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, int max_depth, uint8_t* target, size_t tstride,
                 bool f64, int rgbi, const HostCopy& hc) {
  RtViews vw = c->views;
  const int tiles_y = (a3 + RT_TILE_H - 1) / RT_TILE_H;
  vw.tiles0 = vw.v[0].tiles_x * tiles_y;
  const size_t n_tiles = (size_t)(vw.v[0].tiles_x + vw.v[1].tiles_x) * (size_t)tiles_y;
  if (n_tiles == 0 || n_tiles > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "bad two-eye launch of %zu tiles", n_tiles);
  const dim3 grid((unsigned)n_tiles);
  const int32_t key[8] = {a0, a1, a2, a3, max_depth, f64 ? 1 : 0, c->dev.width, vw.kind};
  rt_ctx::OrderSlot* slot = nullptr;
  bool calibrate = false;
  RT_TRY(acquire_order(c, key, n_tiles, st, &slot, &calibrate));
  const LaunchPlan plan = plan_row_launch(launch_facts(c, max_depth, f64, n_tiles, slot, calibrate));
  const int32_t* order = slot && !calibrate ? slot->d_order : nullptr;
  uint32_t* cost = calibrate ? slot->d_cost : nullptr;
  c->last_kernel = plan.last_kernel;
  if (plan.refused)
    return fail(RT_ERR_UNSUPPORTED, "a pooled kernel for a scene of %d objects (one-byte object index)", c->dev.n_objects);
  if (c->timing) RT_HIP(hipEventRecord(c->ev0, st));
  hipEvent_t mev = nullptr;
#ifndef RT_DIAG_NO_MARKS
  RT_TRY(mark_event(c, st, &mev));
#endif
  if (plan.kind >= 0) {
    void* kargs[] = {&c->dev, &vw, (void*)&a0, (void*)&a1, (void*)&a2, (void*)&a3, &max_depth, &target, &tstride,
                     (void*)&order, &cost, (void*)&rgbi};
    // hipExtModuleLaunchKernel takes the global work size in work-items (grid x 64)
    RT_HIP(hipExtModuleLaunchKernel(spec_fn(c, plan.kind, f64, calibrate), grid.x * 64u, 1, 1, 64, 1, 1, 0, st, kargs,
                                    nullptr, nullptr, mev, 0));
  } else {
    with_mode(plan.mode, [&](auto M) {
      with_flags(f64, calibrate, plan.fc, [&](auto F, auto C, auto K) {
        hipExtLaunchKernelGGL((render_views_kernel<decltype(M)::value, decltype(F)::value, decltype(C)::value, decltype(K)::value>),
                              grid, dim3(RT_WG_THREADS), 0, st, nullptr, mev, 0, c->dev, vw, a0, a1, a2, a3, max_depth, target,
                              tstride, order, cost, rgbi);
      });
    });
  }
  RT_HIP(hipGetLastError());
  RT_TRY(finish_launch(c, st, hc, false));
  // a plain longest-first permutation: no split parts, no XCD line order
  if (calibrate) RT_TRY(finish_calibration(c, st, slot, {c->n_cu * 4.0 * RT_WAVES_MODE(plan.mode), false, false, 0, false, 0, 0}));
  return RT_OK;
}

}  // namespace rt
