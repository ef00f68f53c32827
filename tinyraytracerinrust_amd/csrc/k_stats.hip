// k_stats.hip -- a frame's ray counts (rt_count_rays, rt_count_rays_row_bands): how many get_pixel and
// get_ray_color calls the reference makes for the rows of a band layout, and how many shadow rays it casts,
// per launch, per packed row and per pixel.  These are the reference's ALGORITHMIC counts (raytracer.rs:132-287,
// :359-363; the CPU oracle's C_RAY_* counters), not what the culling render kernels execute: the kernel walks
// every pixel's ray tree with trace() and a recorder that only counts.  The traced colour is never stored, so
// whatever feeds the colour alone is dead code to the compiler; nothing here relies on that.
#include "rt_device.h"
#include "rt_ctx.h"

namespace {

// The launch totals' slots: wave w adds to slot w % RT_COUNT_SLOTS and the host adds the slots up.  Atomics on one
// address are served one after the other: with every wave of the 4K globes launch (129 600) adding to the same four
// words the count took 3.57 ms, 7.4 times the generic frame, and 0.64 ms with the slots.
constexpr int RT_COUNT_SLOTS = 1024;

// The counting recorder (rt_trace.h: trace() reports every get_ray_color call to begin()).  One ray of class
// ray_type per call (RayType: 0 NormalRay, 1 ReflectionRay, 2 TransmissionRay); a ray that hits an object is
// shaded, and shading casts one shadow ray per light whatever the depth (raytracer.rs:175).  finish() is empty,
// so trace()'s slot bookkeeping is dead.  Four counters in registers.
struct CountRec {
  uint32_t primary, shadow, reflect, refract;
  uint32_t n_lights;
  __device__ __forceinline__ int begin(int, int type, V3, V3, double, int oi, V3) {
    primary += type == 0;
    reflect += type == 1;
    refract += type == 2;
    if (oi >= 0) shadow += n_lights;
    return 0;
  }
  __device__ __forceinline__ void finish(int, Col) {}
};

// One wave per 8x8 tile of the launch's packed rows (rt_render_row_bands' geometry; n_rows: the host has dropped
// the rows >= H), one-wave workgroups with the frame stack's first frames in LDS, as aa_trace_kernel.  Lanes
// outside the frame or the owned rows trace nothing and add zeros to the sums.
// VIEWS: a two-eye scene (rt_blob.h RtViews), every pixel's camera ray chosen as get_pixel chooses it
// (k_points.hip render_points_views_kernel): stereoscopic (camera.rs:124-131) x >= W / 2 is the LEFT eye's pixel
// x - W / 2 (view 1), any other the right eye's (view 0); anaglyph (:186-195) both eyes' rays, two traces and two
// primary rays.  Perspective scenes take the instantiation without the branch (and VW is never read).
// Outputs, each optional: pixels -- (primary, shadow, reflect, refract) as one 16-byte store per pixel; rows -- four
// sums per packed row, reduced over a tile row's lanes, one atomic per class and tile row; totals -- four sums of
// the launch, one atomic per class and wave into one of RT_COUNT_SLOTS slots of four (the host adds the slots up).
// Integer adds: exact in any order.
template <bool REFR, bool VIEWS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WAVES(REFR)))) void count_rays_kernel(
    RtDevScene S, RtViews VW, int y_first, int band_rows, int band_pitch, int n_rows, int max_depth,
    unsigned long long* __restrict__ totals, unsigned long long* __restrict__ rows, uint8_t* __restrict__ pixels,
    size_t pixel_stride) {
  constexpr int KLR = REFR ? RT_LDS_RFRAMES : 0;
  __shared__ double s_frames[(RT_LDS_FRAMES * 4 + KLR * 7) * 64 + 1];
  lds_f64* lf = (lds_f64*)&s_frames[threadIdx.x];
  const int lane = threadIdx.x;
  // Workgroups take the tiles column by column: the waves in flight together then lie in different tile rows, so
  // they add to different words of `rows` (row by row, a tile row's waves queue up on its eight rows' sums: 0.94 ms
  // for the 4K globes row sums, 0.48 ms by columns) and a frame's costly rows are spread over the whole launch
  // (the pixel map alone: 0.61 -> 0.46 ms).  The grid is tiles_x * tiles_y workgroups.
  const unsigned tiles_x = (unsigned)(S.width + RT_TILE_W - 1) / RT_TILE_W, tiles_y = gridDim.x / tiles_x;
  const unsigned tile = (blockIdx.x % tiles_y) * tiles_x + blockIdx.x / tiles_y;
  int x, r;
  tile_pixel(tile, lane, S.width, &x, &r);
  bool live = x < S.width && r < n_rows;
  int y = 0;
  if (live) {
    y = band_row(r, y_first, band_rows, band_pitch, n_rows);
    live = y < S.height;
  }
  CountRec R = {0u, 0u, 0u, 0u, (uint32_t)S.n_lights};
  if (live) {
    const DS D = make_ds(S);
    if constexpr (VIEWS) {
      const bool anaglyph = VW.kind == RT_CAMERA_ANAGLYPH;
      int xe = x, eye = 0;
      if (!anaglyph && x >= VW.stereo_w) { xe = x - VW.stereo_w; eye = 1; }
#pragma unroll 1
      for (int k = 0; k < (anaglyph ? 2 : 1); ++k) {
        V3 ro, rd;
        camera_ray(VW.v[anaglyph ? k : eye].cam, (double)xe, (double)y, &ro, &rd);
        (void)trace<REFR, CountRec, RT_LDS_FRAMES, false, KLR>(D, ro, rd, max_depth, &R, lf);
      }
    } else {
      V3 ro, rd;
      camera_ray_px(S, x, y, &ro, &rd);                                     // get_pixel(x as f64, y as f64)
      (void)trace<REFR, CountRec, RT_LDS_FRAMES, false, KLR>(D, ro, rd, max_depth, &R, lf);
    }
    if (pixels) *(uint4*)(pixels + (size_t)r * pixel_stride + (size_t)x * 16) = make_uint4(R.primary, R.shadow, R.reflect, R.refract);
  }
  if (!rows && !totals) return;                                             // wave-uniform
  unsigned long long n[4] = {R.primary, R.shadow, R.reflect, R.refract};
#pragma unroll
  for (int d = 1; d < RT_TILE_W; d <<= 1)                                   // the tile row's lanes
    for (int k = 0; k < 4; ++k) n[k] += __shfl_xor(n[k], d);
  // a tile row's first column is always inside the frame, so its first lane is live exactly when the row is
  if (rows && live && lane % RT_TILE_W == 0)
    for (int k = 0; k < 4; ++k) atomicAdd(rows + (size_t)r * 4 + k, n[k]);
  if (!totals) return;
#pragma unroll
  for (int d = RT_TILE_W; d < 64; d <<= 1)                                  // the wave
    for (int k = 0; k < 4; ++k) n[k] += __shfl_xor(n[k], d);
  if (lane == 0) {
    unsigned long long* slot = totals + (size_t)(blockIdx.x % RT_COUNT_SLOTS) * 4;
    for (int k = 0; k < 4; ++k)
      if (n[k]) atomicAdd(slot + k, n[k]);
  }
}

}  // namespace

using namespace rt;

extern "C" {

// The rows of a band layout, cut to the frame by clamp_bands (launch_plan.h): the kernel sees n_rows packed rows
// that all exist.
int rt_count_rays_row_bands(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                            int32_t max_depth, rt_ray_counts* totals, uint64_t* row_counts, uint32_t* pixel_counts,
                            size_t pixel_stride, void* stream) {
  RT_TRY(side_entry_ok(c, totals || row_counts || pixel_counts, nullptr, &max_depth));
  const int W = c->dev.width;
  const size_t row16 = (size_t)W * 16;
  if (pixel_counts && pixel_stride < row16) return fail(RT_ERR_INVALID, "pixel stride %zu < %zu", pixel_stride, row16);
  if (totals) *totals = {0, 0, 0, 0};
  const BandGeometry g = clamp_bands(W, c->dev.height, y_first, band_rows, band_pitch, n_bands);
  if (g.status == BandGeometry::NOTHING) return RT_OK;
  if (g.status != BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  if (g.n_tiles == 0 || g.n_tiles > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "bad count launch of %zu tiles", g.n_tiles);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  // the row sums and the pixel counts in place or staged; the totals' slots always in the scratch
  const size_t rows_bytes = (size_t)g.n_rows * 32, tot_bytes = (size_t)RT_COUNT_SLOTS * 32;
  Stager sg;
  const int i_rows = sg.add_out(row_counts, rows_bytes, rows_bytes, 1, 8, "row count");
  const int i_px = sg.add_out(pixel_counts, pixel_stride, row16, g.n_rows, 16, "pixel count");
  const int i_tot = totals ? sg.add_scratch(tot_bytes) : -1;
  RT_TRY(sg.reserve(c, st));
  unsigned long long* k_tot = totals ? sg.ptr<unsigned long long>(i_tot) : nullptr;
  unsigned long long* k_rows = sg.ptr<unsigned long long>(i_rows);
  // the sums start at zero, ahead of the timing event: rt_ctx_last_kernel_ms reports the kernel alone
  if (k_tot) RT_HIP(hipMemsetAsync(k_tot, 0, tot_bytes, st));
  if (k_rows) RT_HIP(hipMemsetAsync(k_rows, 0, rows_bytes, st));
  const dim3 grid((unsigned)g.n_tiles);
  const int a0 = (int)g.y_first, a1 = (int)g.band_rows, a2 = (int)g.band_pitch, a3 = (int)g.n_rows;
  RT_TRY(begin_launch(c, st));
  with_bool(c->dev.any_transparent != 0, [&](auto R) {
    with_bool(c->views.kind != 0, [&](auto V) {
      hipLaunchKernelGGL((count_rays_kernel<decltype(R)::value, decltype(V)::value>), grid, dim3(64), 0, st, c->dev, c->views,
                         a0, a1, a2, a3, (int)max_depth, k_tot, k_rows, sg.ptr(i_px), sg.stride(i_px));
    });
  });
  RT_TRY(end_launch(c, st));
  std::vector<unsigned long long> slots(totals ? (size_t)RT_COUNT_SLOTS * 4 : 0);
  if (totals) RT_HIP(hipMemcpyAsync(slots.data(), k_tot, tot_bytes, hipMemcpyDeviceToHost, st));
  RT_TRY(sg.finish(st, totals != nullptr));
  if (totals)
    for (size_t i = 0; i < slots.size(); i += 4) {
      totals->primary += slots[i]; totals->shadow += slots[i + 1]; totals->reflect += slots[i + 2]; totals->refract += slots[i + 3];
    }
  return RT_OK;
}

int rt_count_rays(rt_ctx* c, uint32_t y0, uint32_t y1, int32_t max_depth, rt_ray_counts* totals, uint64_t* row_counts,
                  uint32_t* pixel_counts, size_t pixel_stride_bytes, void* stream) {
  RT_TRY(side_entry_ok(c, totals || row_counts || pixel_counts, nullptr, nullptr));
  if (y0 > y1 || y1 > (uint32_t)c->dev.height) return fail(RT_ERR_INVALID, "bad row range [%u, %u) for height %d", y0, y1, c->dev.height);
  return rt_count_rays_row_bands(c, y0, y1 - y0, y1 - y0, 1, max_depth, totals, row_counts, pixel_counts, pixel_stride_bytes, stream);
}

}  // extern "C"
