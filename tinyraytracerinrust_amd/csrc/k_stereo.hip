// k_stereo.hip -- the row kernels of two-eye scenes: StereoscopicCamera (raytracer/camera.rs:82-141: two
// eyes side by side in one frame) and AnaglyphCamera (:143-205: red from the left eye, green and blue from
// the right).  A two-eye frame is the rays of two perspective frames, so it is ONE launch over the tiles
// of two views (rt_blob.h RtViews, rt_device.h rows_views_body): one wave per (view, 8x8 tile of that
// view), the camera wave-uniform, trace() and its register budget those of the perspective megakernels,
// every output byte written once.  The perspective kernels (k_rows.hip) take no part and no new branch.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

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

// launch_bands' threshold (k_rows.hip): launches of fewer entries are dispatched in entry order
#ifndef RT_ORDER_MIN_TILES
#define RT_ORDER_MIN_TILES 2048
#endif

namespace rt {

// A two-eye scene's row launch.  The entries are view 0's tiles, then view 1's; the longest-first order
// and its calibration (launch_bands) run over all of them, from RT_ORDER_MIN_TILES entries.  Always the
// view megakernel of the scene's mode, generic or specialised: RT_OPT_KERNEL's deferred and wavefront
// choices and the tile masks have no two-eye form.
int launch_views(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, int max_depth, uint8_t* target, size_t tstride,
                 bool f64, int rgbi, void* host_out, size_t host_stride, size_t row_bytes) {
  RtViews vw = c->views;
  const int tiles_y = (a3 + RT_TILE_H - 1) / RT_TILE_H;
  vw.tiles0 = vw.v[0].tiles_x * tiles_y;
  const size_t n_tiles = (size_t)(vw.v[0].tiles_x + vw.v[1].tiles_x) * (size_t)tiles_y;
  if (n_tiles == 0 || n_tiles > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "bad two-eye launch of %zu tiles", n_tiles);
  dim3 grid((unsigned)n_tiles), block(RT_WG_THREADS);
  const int32_t key[8] = {a0, a1, a2, a3, max_depth, f64 ? 1 : 0, c->dev.width, vw.kind};
  rt_ctx::OrderSlot* slot = nullptr;
  bool calibrate = false;
  if (c->tile_order && n_tiles >= RT_ORDER_MIN_TILES) {
    for (auto& s : c->order)
      if (s.valid && memcmp(s.key, key, sizeof(key)) == 0) slot = &s;
    if (!slot) {                      // calibrate into the empty or least recently used slot
      slot = &c->order[0];
      for (auto& s : c->order) {
        if (!s.valid) { slot = &s; break; }
        if (s.last_use < slot->last_use) slot = &s;
      }
      drop_order(*slot);
      RT_HIP(hipMalloc((void**)&slot->d_order, n_tiles * sizeof(int32_t)));
      RT_HIP(hipMalloc((void**)&slot->d_cost, n_tiles * sizeof(uint32_t)));
      RT_HIP(hipMemsetAsync(slot->d_cost, 0, n_tiles * sizeof(uint32_t), st));   // tiles that store no cost sort last
      memcpy(slot->key, key, sizeof(key));
      slot->n_tiles = n_tiles;
      slot->grid = (uint32_t)n_tiles;
      calibrate = true;
    }
    slot->last_use = ++c->use_clock;
  }
  const int32_t* order = slot && !calibrate ? slot->d_order : nullptr;
  uint32_t* cost = calibrate ? slot->d_cost : nullptr;
  if (c->timing) RT_HIP(hipEventRecord(c->ev0, st));
  hipEvent_t mev = nullptr;
#ifndef RT_DIAG_NO_MARKS
  RT_TRY(mark_event(c, st, &mev));
#endif
  const bool refr = c->dev.any_transparent != 0, chain = refr && c->dev.ray_chains != 0;
  const bool fc = c->dev.colour_fast != 0 && c->fast_clamp;
  const int mode = chain ? RT_MODE_CHAIN : refr ? RT_MODE_TREE : RT_MODE_REFL;
  // the pooled modes hold the hit object in one byte (launch_bands' check)
  const bool pooled = mode == RT_MODE_CHAIN || (mode == RT_MODE_REFL && RT_LDS_POOL_REFL > 0);
  if (pooled && RT_POOL_OBJ_INDEX && c->dev.n_objects > 256)
    return fail(RT_ERR_UNSUPPORTED, "a pooled kernel for a scene of %d objects (one-byte object index)", c->dev.n_objects);
  hipFunction_t sfn = nullptr;
  if (c->spec.prog.two_eyes && mode == c->spec.prog.mode && fc == c->spec.prog.fc) sfn = spec_fn(c, SPEC_VIEWS, f64, calibrate);
  c->last_kernel = sfn ? "view megakernel (specialised)" : "view megakernel";
  if (sfn) {
    void* kargs[] = {&c->dev, &vw, (void*)&a0, (void*)&a1, (void*)&a2, (void*)&a3, &max_depth, &target, &tstride,
                     (void*)&order, &cost, (void*)&rgbi};
    // hipExtModuleLaunchKernel takes the global work size in work-items (grid x 64)
    RT_HIP(hipExtModuleLaunchKernel(sfn, grid.x * 64u, 1, 1, 64, 1, 1, 0, st, kargs, nullptr, nullptr, mev, 0));
  } else {
#define RT_LAUNCH_VIEWS(M, F, C, K)                                                                              \
  hipExtLaunchKernelGGL((render_views_kernel<M, F, C, K>), grid, block, 0, st, nullptr, mev, 0, c->dev, vw, a0, a1, a2, \
                        a3, max_depth, target, tstride, order, cost, rgbi)
#define RT_LAUNCH_VIEWS_M(M)                                                           \
  if (f64 && calibrate && fc) RT_LAUNCH_VIEWS(M, true, true, true);                    \
  else if (f64 && calibrate) RT_LAUNCH_VIEWS(M, true, true, false);                    \
  else if (f64 && fc) RT_LAUNCH_VIEWS(M, true, false, true);                           \
  else if (f64) RT_LAUNCH_VIEWS(M, true, false, false);                                \
  else if (calibrate && fc) RT_LAUNCH_VIEWS(M, false, true, true);                     \
  else if (calibrate) RT_LAUNCH_VIEWS(M, false, true, false);                          \
  else if (fc) RT_LAUNCH_VIEWS(M, false, false, true);                                 \
  else RT_LAUNCH_VIEWS(M, false, false, false);
    if (mode == RT_MODE_CHAIN) { RT_LAUNCH_VIEWS_M(RT_MODE_CHAIN) }
    else if (mode == RT_MODE_TREE) { RT_LAUNCH_VIEWS_M(RT_MODE_TREE) }
    else { RT_LAUNCH_VIEWS_M(RT_MODE_REFL) }
#undef RT_LAUNCH_VIEWS_M
#undef RT_LAUNCH_VIEWS
  }
  RT_HIP(hipGetLastError());
  if (c->timing) RT_HIP(hipEventRecord(c->ev1, st));
  c->timed = c->timing;
  if (calibrate) {                    // synchronous, once per geometry and scene upload: longest first
    std::vector<uint32_t> h_cost(n_tiles);
    std::vector<int32_t> h_order(n_tiles);
    RT_HIP(hipMemcpyAsync(h_cost.data(), slot->d_cost, n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < n_tiles; ++i) h_order[i] = (int32_t)i;
    std::stable_sort(h_order.begin(), h_order.end(), [&](int32_t x, int32_t y) { return h_cost[x] > h_cost[y]; });
    RT_HIP(hipMemcpyAsync(slot->d_order, h_order.data(), n_tiles * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RT_HIP(hipStreamSynchronize(st));
    slot->valid = true;
  }
  if (host_out) {
    RT_HIP(hipMemcpy2DAsync(host_out, host_stride, target, tstride, row_bytes, (size_t)a3, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
  }
  return RT_OK;
}

}  // namespace rt
