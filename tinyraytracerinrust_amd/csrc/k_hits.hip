// k_hits.hip -- first-hit maps (rt_first_hits, rt_first_hits_row_bands, rt_first_hits_points): per pixel of the
// rows of a band layout, or per sample position, the object the camera ray hits first, the hit distance, which
// lights' shadow rays are occluded there and the shape's raw normal -- the questions a host asks about a frame
// before any shading (picking, depth / id / normal passes, shadow overlays).  The per-sample function is
// rt_hits.h's first_hit: the render kernels' own walks, nothing of their shading, nothing that recurses.
#include "rt_device.h"
#include "rt_hits.h"
#include "rt_ctx.h"

namespace {

// The four output planes as the kernels take them: rt_hit_planes with byte pointers (null: not asked for).
struct HitPlanes {
  uint8_t* object;   size_t object_stride;
  uint8_t* distance; size_t distance_stride;
  uint8_t* shadow;   size_t shadow_stride;
  uint8_t* normal;   size_t normal_stride;
};

// Waves per SIMD: with no pin the instantiations take 52 to 79 VGPRs (reflection-only walks: 52 for id and depth,
// 67 with the shadow walk; the refraction walks' shared sphere terms: 64 and 79; DESIGN.md section 6 "First-hit
// maps"), none spills, none uses scratch or LDS.  So the kernels carry NO amdgpu_waves_per_eu: the frame-stack
// kernels' pins (4 and 5 waves) trade registers against their LDS frames, and there are none here; a pin above
// what the register count gives (8 waves = 64 VGPRs) would make the shadow forms spill for walks that already
// run at 6 or 7 waves, and one below would only idle slots.  Each instantiation runs at its own count's occupancy.

// One wave per 8x8 tile of the launch's packed rows (rt_render_row_bands' geometry; n_rows: the host has dropped
// the rows >= H), one-wave workgroups, tiles row-major; no frame stack, no LDS.  Lanes outside the frame or the
// owned rows do nothing.  VIEWS: a stereoscopic scene (rt_blob.h RtViews), the camera ray chosen as get_pixel
// chooses it (camera.rs:124-131, count_rays_kernel): x >= W / 2 is the LEFT eye's pixel x - W / 2 (view 1), any
// other the right eye's (view 0); perspective scenes take the instantiation without the branch.
// Stores: one per plane per lane, plain (the host or another kernel reads the planes next); a tile row's 8 lanes
// write 32 contiguous bytes of the object and shadow planes, 64 of the distance plane and 192 of the normals.
template <bool REFR, bool SHADOW, bool NORMAL, bool VIEWS>
__global__ __launch_bounds__(64) void first_hits_kernel(RtDevScene S, RtViews VW, int y_first, int band_rows,
                                                        int band_pitch, int n_rows, HitPlanes P) {
  const int lane = threadIdx.x;
  int x, r;
  tile_pixel(blockIdx.x, lane, S.width, &x, &r);
  if (x >= S.width || r >= n_rows) return;
  const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
  if (y >= S.height) return;
  V3 ro, rd;
  if constexpr (VIEWS) {
    int xe = x, eye = 0;
    if (x >= VW.stereo_w) { xe = x - VW.stereo_w; eye = 1; }
    camera_ray(VW.v[eye].cam, (double)xe, (double)y, &ro, &rd);
  } else {
    camera_ray_px(S, x, y, &ro, &rd);                                      // get_pixel(x as f64, y as f64)
  }
  const FirstHit h = first_hit<REFR, SHADOW, NORMAL>(make_ds(S), ro, rd);
  if (P.object) *(int32_t*)(P.object + (size_t)r * P.object_stride + (size_t)x * 4) = h.object;
  if (P.distance) *(double*)(P.distance + (size_t)r * P.distance_stride + (size_t)x * 8) = h.distance;
  if constexpr (SHADOW) *(uint32_t*)(P.shadow + (size_t)r * P.shadow_stride + (size_t)x * 4) = h.shadow;
  if constexpr (NORMAL) {
    double* n = (double*)(P.normal + (size_t)r * P.normal_stride + (size_t)x * 24);
    n[0] = h.normal.x; n[1] = h.normal.y; n[2] = h.normal.z;
  }
}

// The same per sample position: n (x, y) pairs, contiguous outputs (null: not asked for; shadow and normal are
// non-null exactly when SHADOW / NORMAL).  The camera as render_points_kernel / render_points_views_kernel:
// stereoscopic x >= W / 2 (as f64) is the left eye's sample at x - W / 2.
template <bool REFR, bool SHADOW, bool NORMAL, bool VIEWS>
__global__ __launch_bounds__(256) void first_hits_points_kernel(RtDevScene S, RtViews VW, const double* __restrict__ xy,
                                                                size_t n, int32_t* __restrict__ object,
                                                                double* __restrict__ distance,
                                                                uint32_t* __restrict__ shadow, double* __restrict__ normal) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 ro, rd;
  if constexpr (VIEWS) {
    const double w = (double)VW.stereo_w;
    double x = xy[2 * i];
    int eye = 0;
    if (x >= w) { x = x - w; eye = 1; }
    camera_ray(VW.v[eye].cam, x, xy[2 * i + 1], &ro, &rd);
  } else {
    camera_ray(S.cam, xy[2 * i], xy[2 * i + 1], &ro, &rd);
  }
  const FirstHit h = first_hit<REFR, SHADOW, NORMAL>(make_ds(S), ro, rd);
  if (object) object[i] = h.object;
  if (distance) distance[i] = h.distance;
  if constexpr (SHADOW) shadow[i] = h.shadow;
  if constexpr (NORMAL) { normal[3 * i] = h.normal.x; normal[3 * i + 1] = h.normal.y; normal[3 * i + 2] = h.normal.z; }
}

}  // namespace

using namespace rt;

// f(REFR, SHADOW, NORMAL, VIEWS) as std::bool_constant values: each combination instantiated once
template <class F>
static void with_hit_flags(bool refr, bool shadow, bool normal, bool views, F&& f) {
  with_bool(refr, [&](auto R) {
    with_bool(shadow, [&](auto Sh) { with_bool(normal, [&](auto N) { with_bool(views, [&](auto V) { f(R, Sh, N, V); }); }); });
  });
}

// What every entry checks before its geometry: the side entries' refusals, the camera kind, the shadow bits' room.
static int hits_scene_ok(rt_ctx* c, bool args, bool shadow) {
  RT_TRY(side_entry_ok(c, args, nullptr, nullptr));
  if (c->views.kind == RT_CAMERA_ANAGLYPH) return fail(RT_ERR_UNSUPPORTED, "first hits of an anaglyph scene: a pixel has two, one per eye");
  if (shadow && c->dev.n_lights > 32) return fail(RT_ERR_UNSUPPORTED, "shadow bits of %d lights > 32", c->dev.n_lights);
  return RT_OK;
}

extern "C" {

// The rows of a band layout, cut to the frame by clamp_bands (launch_plan.h): the kernel sees n_rows packed rows
// that all exist.
int rt_first_hits_row_bands(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                            const rt_hit_planes* out, void* stream) {
  RT_TRY(hits_scene_ok(c, out && (out->object || out->distance || out->shadow || out->normal), out && out->shadow));
  const int W = c->dev.width;
  struct Plane { void* p; size_t stride, px; const char* what; };
  const Plane pl[4] = {{out->object, out->object_stride, 4, "object"}, {out->distance, out->distance_stride, 8, "distance"},
                       {out->shadow, out->shadow_stride, 4, "shadow"}, {out->normal, out->normal_stride, 24, "normal"}};
  for (const Plane& q : pl)
    if (q.p && q.stride < q.px * (size_t)W) return fail(RT_ERR_INVALID, "%s stride %zu < %zu", q.what, q.stride, q.px * (size_t)W);
  const BandGeometry g = clamp_bands(W, c->dev.height, y_first, band_rows, band_pitch, n_bands);
  if (g.status == BandGeometry::NOTHING) return RT_OK;
  if (g.status != BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  if (g.n_tiles == 0 || g.n_tiles > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "bad first-hit launch of %zu tiles", g.n_tiles);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  // device planes are written in place (element-aligned rows); host planes are staged, packed, in the scratch
  Stager sg;
  for (const Plane& q : pl) sg.add_out(q.p, q.stride, q.px * (size_t)W, g.n_rows, q.px == 4 ? 4 : 8, q.what);
  RT_TRY(sg.reserve(c, st));
  const HitPlanes P = {sg.ptr(0), sg.stride(0), sg.ptr(1), sg.stride(1), sg.ptr(2), sg.stride(2), sg.ptr(3), sg.stride(3)};
  const dim3 grid((unsigned)g.n_tiles);
  const int a0 = (int)g.y_first, a1 = (int)g.band_rows, a2 = (int)g.band_pitch, a3 = (int)g.n_rows;
  RT_TRY(begin_launch(c, st));
  with_hit_flags(c->dev.any_transparent != 0, P.shadow != nullptr, P.normal != nullptr, c->views.kind != 0,
                 [&](auto R, auto Sh, auto N, auto V) {
    hipLaunchKernelGGL((first_hits_kernel<decltype(R)::value, decltype(Sh)::value, decltype(N)::value, decltype(V)::value>),
                       grid, dim3(64), 0, st, c->dev, c->views, a0, a1, a2, a3, P);
  });
  RT_TRY(end_launch(c, st));
  return sg.finish(st, false);
}

int rt_first_hits(rt_ctx* c, uint32_t y0, uint32_t y1, const rt_hit_planes* out, void* stream) {
  RT_TRY(side_entry_ok(c, out && (out->object || out->distance || out->shadow || out->normal), nullptr, nullptr));
  if (y0 > y1 || y1 > (uint32_t)c->dev.height) return fail(RT_ERR_INVALID, "bad row range [%u, %u) for height %d", y0, y1, c->dev.height);
  return rt_first_hits_row_bands(c, y0, y1 - y0, y1 - y0, 1, out, stream);
}

int rt_first_hits_points(rt_ctx* c, const double* xy, size_t n, int32_t* object, double* distance, uint32_t* shadow,
                         double* normal, void* stream) {
  RT_TRY(hits_scene_ok(c, xy && (object || distance || shadow || normal), shadow != nullptr));
  if (n == 0) return RT_OK;
  if (n > (size_t)INT32_MAX) return fail(RT_ERR_INVALID, "%zu sample positions > %d", n, INT32_MAX);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  // device arrays are read and written in place (element-aligned); host arrays are staged in the scratch
  void* const outs[4] = {object, distance, shadow, normal};
  const size_t px[4] = {4, 8, 4, 24};
  const char* const what[4] = {"object", "distance", "shadow", "normal"};
  Stager sg;
  for (int k = 0; k < 4; ++k) sg.add_out(outs[k], n * px[k], n * px[k], 1, px[k] == 4 ? 4 : 8, what[k]);
  const int k_xy = sg.add_in(xy, n * 16, n * 16, 1, 8, "sample position");
  RT_TRY(sg.reserve(c, st));
  const double* in = sg.ptr<const double>(k_xy);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  RT_TRY(begin_launch(c, st));
  with_hit_flags(c->dev.any_transparent != 0, shadow != nullptr, normal != nullptr, c->views.kind != 0,
                 [&](auto R, auto Sh, auto N, auto V) {
    hipLaunchKernelGGL((first_hits_points_kernel<decltype(R)::value, decltype(Sh)::value, decltype(N)::value, decltype(V)::value>),
                       grid, block, 0, st, c->dev, c->views, in, n, sg.ptr<int32_t>(0), sg.ptr<double>(1), sg.ptr<uint32_t>(2),
                       sg.ptr<double>(3));
  });
  RT_TRY(end_launch(c, st));
  return sg.finish(st, false);
}

}  // extern "C"
