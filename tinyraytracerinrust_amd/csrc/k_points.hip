// k_points.hip -- scene-level get_pixel at any (x, y) (rt_render_points_f64, rt_trace_pixel_f64;
// raytracer.rs:359-363), the path the parity tests' chosen points take.  Its own translation unit so
// that its traversals cull with the specialised programs' f32 slab tests (RT_CULL_F32, rt_device.h
// fbox_may_hit) on the same outward-rounded boxes: the edge tests (tests/test_gpu_cull_edges.py,
// test_gpu_texel_boundary.py) aim rays at silhouettes and shadow edges -- the culling decisions closest
// to a box -- through this kernel.  A context whose scene has a specialised points kernel loaded (spec_text.cpp
// rt_spec_points, RT_OPT_SPEC_SAMPLES) launches that instead: the specialised programs' own walks, which
// tests/test_gpu_spec_samples.py aims the same rays at.
#ifndef RT_CULL_F32
#define RT_CULL_F32 1
#endif
#include "rt_device.h"
#include "rt_ctx.h"

namespace {

template <bool REFR>
__global__ __launch_bounds__(256) void render_points_kernel(RtDevScene S, const double* __restrict__ xy,
                                                            size_t n, int max_depth, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 ro, rd;
  camera_ray(S.cam, xy[2 * i], xy[2 * i + 1], &ro, &rd);
  const Col c = trace<REFR>(make_ds(S), ro, rd, max_depth);
  out[4 * i] = c.r; out[4 * i + 1] = c.g; out[4 * i + 2] = c.b; out[4 * i + 3] = 1.0;
}

// The same for a two-eye scene (rt_blob.h RtViews).  Stereoscopic (camera.rs:124-131): a sample at
// x >= W / 2 (as f64) is the LEFT eye's at x - W / 2 (view 1), any other the right eye's at x (view 0).
// Anaglyph (:186-195): both eyes' rays at (x, y), view 0 (left) giving r, view 1 (right) g and b.
template <bool REFR>
__global__ __launch_bounds__(256) void render_points_views_kernel(RtDevScene S, RtViews VW, const double* __restrict__ xy,
                                                                  size_t n, int max_depth, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool anaglyph = VW.kind == RT_CAMERA_ANAGLYPH;
  const double w = (double)VW.stereo_w, y = xy[2 * i + 1];
  double x = xy[2 * i];
  int eye = 0;
  if (!anaglyph && x >= w) { x = x - w; eye = 1; }
#pragma unroll 1
  for (int k = 0; k < (anaglyph ? 2 : 1); ++k) {
    V3 ro, rd;
    camera_ray(VW.v[anaglyph ? k : eye].cam, x, y, &ro, &rd);
    const Col c = trace<REFR>(make_ds(S), ro, rd, max_depth);
    if (!anaglyph || k == 0) out[4 * i] = c.r;
    if (!anaglyph || k == 1) { out[4 * i + 1] = c.g; out[4 * i + 2] = c.b; out[4 * i + 3] = 1.0; }
  }
}

}  // namespace

using namespace rt;

extern "C" {

int rt_trace_pixel_f64(const rt_scene* scene, double x, double y, int32_t max_depth, int device, double rgba[4]) {
  if (!scene || !rgba) return fail(RT_ERR_INVALID, "null argument");
  struct Holder {                       // the calling thread's context, freed with the thread
    rt_ctx* c = nullptr;
    ~Holder() { if (c) rt_ctx_free(c); }
  };
  static thread_local Holder h;
  if (h.c && h.c->device != device) {
    rt_ctx_free(h.c);
    h.c = nullptr;
  }
  if (!h.c) {
    int rc = rt_ctx_create(device, &h.c);
    if (rc) return rc;
    rt_ctx_set_option(h.c, RT_OPT_TIMING, 0);
    rt_ctx_set_option(h.c, RT_OPT_SPECIALIZE, 0);   // one point per upload: never worth a compile
  }
  int rc = rt_ctx_upload(h.c, scene);
  if (rc) return rc;
  const double xy[2] = {x, y};
  return rt_render_points_f64(h.c, xy, 1, max_depth, rgba, nullptr);
}

int rt_render_points_f64(rt_ctx* c, const double* xy, size_t n, int32_t max_depth, double* out, void* stream) {
  RT_TRY(side_entry_ok(c, xy && out, nullptr, &max_depth));
  if (n == 0) return RT_OK;
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  Stager sg;
  const int i_in = sg.add_in(xy, n * 16, n * 16, 1, 0, "sample position"), i_out = sg.add_out(out, n * 32, n * 32, 1, 0, "output");
  RT_TRY(sg.reserve(c, st));
  const double* in = sg.ptr<const double>(i_in);
  double* target = sg.ptr<double>(i_out);
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  // the scene's specialised points kernel (spec_text.cpp rt_spec_points: one-wave workgroups), once it is loaded;
  // a launch of 2^31 samples or more keeps the generic kernel (the module launch's work size is 32 bits)
  hipFunction_t sfn = spec_sample_kernel(c, SPEC_POINTS);
  if (sfn && n >= ((size_t)1 << 31)) {
    sfn = nullptr;
    c->spec.last_sample = "points";
  }
  RT_TRY(begin_launch(c, st));
  if (sfn) {
    int depth = max_depth;
    void* kargs[] = {&c->dev, (void*)&in, &n, &depth, &target};
    RT_HIP(hipModuleLaunchKernel(sfn, (unsigned)((n + 63) / 64), 1, 1, 64, 1, 1, 0, st, kargs, nullptr));
  }
  else
    with_bool(c->dev.any_transparent != 0, [&](auto R) {
      if (c->views.kind) hipLaunchKernelGGL((render_points_views_kernel<decltype(R)::value>), grid, block, 0, st, c->dev, c->views, in, n, max_depth, target);
      else hipLaunchKernelGGL((render_points_kernel<decltype(R)::value>), grid, block, 0, st, c->dev, in, n, max_depth, target);
    });
  RT_TRY(end_launch(c, st));
  return sg.finish(st, false);
}

}  // extern "C"
