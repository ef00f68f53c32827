// k_stats.hip -- a frame's ray counts (rt_count_rays, rt_count_rays_row_bands): how many get_pixel and
// get_ray_color calls the reference makes for the rows of a band layout, and how many shadow rays it casts,
// per launch, per packed row and per pixel.  These are the reference's ALGORITHMIC counts (raytracer.rs:132-287,
// :359-363; the CPU oracle's C_RAY_* counters), not what the culling render kernels execute: the kernel walks
// every pixel's ray tree with trace() and a recorder that only counts.  The traced colour is never stored, so
// whatever feeds the colour alone is dead code to the compiler; nothing here relies on that.
#include <algorithm>

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

// The rows of a band layout, checked and clamped as rt_antialias_row_bands does (k_views.hip antialias_rows): the
// kernel sees n_rows packed rows that all exist.
static int count_rows(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                      int32_t max_depth, rt_ray_counts* totals, uint64_t* row_counts, uint32_t* pixel_counts,
                      size_t pixel_stride, void* stream) {
  if (!c || (!totals && !row_counts && !pixel_counts)) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (max_depth < 0) max_depth = c->max_depth;
  if (max_depth > RT_MAX_DEPTH_CAP) return fail(RT_ERR_UNSUPPORTED, "max_depth %d > %d", max_depth, RT_MAX_DEPTH_CAP);
  const int W = c->dev.width, H = c->dev.height;
  const size_t row16 = (size_t)W * 16;
  if (pixel_counts && pixel_stride < row16) return fail(RT_ERR_INVALID, "pixel stride %zu < %zu", pixel_stride, row16);
  if (totals) *totals = {0, 0, 0, 0};
  if (band_rows == 0 || n_bands == 0) return RT_OK;
  if (band_pitch < band_rows && n_bands > 1) return fail(RT_ERR_INVALID, "band pitch %u < band rows %u", band_pitch, band_rows);
  if (y_first >= (uint32_t)H) return fail(RT_ERR_INVALID, "first row %u >= height %d", y_first, H);
  if (n_bands > 1) n_bands = std::min(n_bands, ((uint32_t)H - 1 - y_first) / band_pitch + 1);
  const uint32_t last_rows = std::min(band_rows, (uint32_t)H - (y_first + (n_bands - 1) * band_pitch));
  if (n_bands == 1) band_rows = band_pitch = last_rows;
  const uint32_t n_rows = (n_bands - 1) * band_rows + last_rows;
  const size_t n_tiles = (size_t)((W + RT_TILE_W - 1) / RT_TILE_W) * ((n_rows + RT_TILE_H - 1) / RT_TILE_H);
  if (n_tiles == 0 || n_tiles > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "bad count launch of %zu tiles", n_tiles);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  const bool d_rows = !row_counts || is_device_ptr(row_counts), d_px = !pixel_counts || is_device_ptr(pixel_counts);
  if (row_counts && d_rows && ((uintptr_t)row_counts & 7)) return fail(RT_ERR_INVALID, "row counts must be 8-byte aligned");
  if (pixel_counts && d_px && (((uintptr_t)pixel_counts | pixel_stride) & 15))
    return fail(RT_ERR_INVALID, "pixel count rows must be 16-byte aligned");
  // device staging: [the totals' slots][row sums][pixel counts], the last two for host pointers
  const size_t rows_bytes = (size_t)n_rows * 32;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t tot_bytes = (size_t)RT_COUNT_SLOTS * 32;
  const size_t o_tot = totals ? take(tot_bytes) : 0, o_rows = d_rows ? 0 : take(rows_bytes), o_px = d_px ? 0 : take(row16 * n_rows);
  if (off) RT_TRY(ensure_scratch(c, off));
  uint8_t* sb = (uint8_t*)c->scratch;
  unsigned long long* k_tot = totals ? (unsigned long long*)(sb + o_tot) : nullptr;
  unsigned long long* k_rows = row_counts ? (unsigned long long*)(d_rows ? (uint8_t*)row_counts : sb + o_rows) : nullptr;
  uint8_t* k_px = pixel_counts ? (d_px ? (uint8_t*)pixel_counts : sb + o_px) : nullptr;
  const size_t k_stride = d_px ? pixel_stride : row16;
  // the sums start at zero, ahead of the timing event: rt_ctx_last_kernel_ms reports the kernel alone
  if (k_tot) RT_HIP(hipMemsetAsync(k_tot, 0, tot_bytes, st));
  if (k_rows) RT_HIP(hipMemsetAsync(k_rows, 0, rows_bytes, st));
  const dim3 grid((unsigned)n_tiles);
  const int a0 = (int)y_first, a1 = (int)band_rows, a2 = (int)band_pitch, a3 = (int)n_rows;
  if (c->timing) RT_HIP(hipEventRecord(c->ev0, st));
  with_bool(c->dev.any_transparent != 0, [&](auto R) {
    with_bool(c->views.kind != 0, [&](auto V) {
      hipLaunchKernelGGL((count_rays_kernel<decltype(R)::value, decltype(V)::value>), grid, dim3(64), 0, st, c->dev, c->views,
                         a0, a1, a2, a3, (int)max_depth, k_tot, k_rows, k_px, k_stride);
    });
  });
  RT_HIP(hipGetLastError());
  if (c->timing) RT_HIP(hipEventRecord(c->ev1, st));
  c->timed = c->timing;
  RT_TRY(mark_launch(c, st));
  std::vector<unsigned long long> slots(totals ? (size_t)RT_COUNT_SLOTS * 4 : 0);
  if (totals) RT_HIP(hipMemcpyAsync(slots.data(), k_tot, tot_bytes, hipMemcpyDeviceToHost, st));
  if (!d_rows) RT_HIP(hipMemcpyAsync(row_counts, k_rows, rows_bytes, hipMemcpyDeviceToHost, st));
  if (!d_px) RT_HIP(hipMemcpy2DAsync(pixel_counts, pixel_stride, k_px, row16, row16, n_rows, hipMemcpyDeviceToHost, st));
  if (totals || !d_rows || !d_px) RT_HIP(hipStreamSynchronize(st));
  if (totals)
    for (size_t i = 0; i < slots.size(); i += 4) {
      totals->primary += slots[i]; totals->shadow += slots[i + 1]; totals->reflect += slots[i + 2]; totals->refract += slots[i + 3];
    }
  return RT_OK;
}

extern "C" {

int rt_count_rays_row_bands(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                            int32_t max_depth, rt_ray_counts* totals, uint64_t* row_counts, uint32_t* pixel_counts,
                            size_t pixel_stride_bytes, void* stream) {
  return count_rows(c, y_first, band_rows, band_pitch, n_bands, max_depth, totals, row_counts, pixel_counts,
                    pixel_stride_bytes, stream);
}

int rt_count_rays(rt_ctx* c, uint32_t y0, uint32_t y1, int32_t max_depth, rt_ray_counts* totals, uint64_t* row_counts,
                  uint32_t* pixel_counts, size_t pixel_stride_bytes, void* stream) {
  if (!c || (!totals && !row_counts && !pixel_counts)) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (y0 > y1 || y1 > (uint32_t)c->dev.height) return fail(RT_ERR_INVALID, "bad row range [%u, %u) for height %d", y0, y1, c->dev.height);
  return count_rows(c, y0, y1 - y0, y1 - y0, 1, max_depth, totals, row_counts, pixel_counts, pixel_stride_bytes, stream);
}

}  // extern "C"
