// k_ortho.hip -- the orthogonal preview views (rt_render_ortho), behind the same C ABI as the row loop.
// DebugWindow::render_orthogonal_view_line (debug_window.rs:166-227): a ray from 10000 along the
// view axis per pixel; the object with the smallest intersection distance -- ANY sign, no EPS,
// strict `<` so the first emitted wins ties -- gives its flat colour (RTObject::get_color =
// material colour at uv (0,0), rt_object.rs:45-47); a miss is Color::EMPTY.  No culling: t may
// be negative.
#include "rt_device.h"
#include "rt_ctx.h"

namespace {

struct OrthoView { int axis1, axis2, axis3; double dir1, dir2, scale; };

__global__ __launch_bounds__(256) void ortho_kernel(RtDevScene S, OrthoView V, int y0, int n_rows,
                                                    uint8_t* __restrict__ out, size_t stride,
                                                    double* __restrict__ f64, size_t f64_stride) {
  int x, r;
  tile16_pixel(blockIdx.x, threadIdx.x, S.width, &x, &r);
  if (x >= S.width || r >= n_rows) return;
  const int y = y0 + r;
  const DS D = make_ds(S);
  const double cx = (double)S.width / 2.0, cy = (double)S.height / 2.0;
  double o3[3] = {0.0, 0.0, 0.0}, d3[3] = {0.0, 0.0, 0.0};
  o3[V.axis1] = (((double)x - cx) * V.dir1) / V.scale;
  o3[V.axis2] = (((double)y - cy) * V.dir2) / V.scale;
  o3[V.axis3] = 10000.0;
  d3[V.axis3] = 1.0;
  const V3 ro = {o3[0], o3[1], o3[2]}, rd = {d3[0], d3[1], d3[2]};
  double best = INFINITY;
  int bobj = -1;
  const bool fin = wave_finite(ro, rd);
  for (int o = 0; o < D.n_objects; ++o) {
    cptr<RtObject> O = &D.objects[o];
    const int lb = O->leaf_begin, le = lb + O->leaf_count;
    for (int l = lb; l < le; ++l) {
      cptr<RtLeaf> L = &D.leaves[l];
      double t0 = 0.0, t1 = 0.0;
      const int n = leaf_candidates(L, ro, rd, fin, &t0, &t1);
      const bool filtered = L->prog_end != L->prog_begin;
      if (n >= 1 && t0 < best && (!filtered || leaf_filter(D, L, add(ro, scale(rd, t0))))) { best = t0; bobj = o; }
      if (n >= 2 && t1 < best && (!filtered || leaf_filter(D, L, add(ro, scale(rd, t1))))) { best = t1; bobj = o; }
    }
  }
  double c[4] = {0.0, 0.0, 0.0, 0.0};                                     // Color::EMPTY
  if (bobj >= 0) {
    cptr<RtObject> O = &D.objects[bobj];
    if (O->textured) {                                                     // texture.rs:27-34 at (0, 0)
      const int tw = D.textures[O->tex].w, th = D.textures[O->tex].h;
      const double ty = (double)th - (0.0 * (double)(th - 1)) - 1.0;
      const int yi = ty > 0.0 ? (ty < (double)(th - 1) ? (int)ty : th - 1) : 0;
      const uint32_t px = *(const uint32_t*)(D.texels + D.textures[O->tex].offset + (size_t)yi * tw * 4);
      c[0] = (double)(px & 0xffu) / 255.0; c[1] = (double)((px >> 8) & 0xffu) / 255.0;
      c[2] = (double)((px >> 16) & 0xffu) / 255.0; c[3] = (double)(px >> 24) / 255.0;
    } else {
      c[0] = O->color[0]; c[1] = O->color[1]; c[2] = O->color[2]; c[3] = O->color_a;
    }
  }
  put_rgba(c[0], c[1], c[2], c[3], x, r, out, stride, f64, f64_stride);
}

}  // namespace

using namespace rt;

extern "C" {

// debug_window.rs:166-227 for rows [y0, y1) of the scene's frame size.
int rt_render_ortho(rt_ctx* c, int32_t axis1, int32_t axis2, double dir1, double dir2, double scale, uint32_t y0,
                    uint32_t y1, uint8_t* rgba8, size_t row_stride_bytes, double* rgba_f64, size_t f64_stride,
                    void* stream) {
  RT_TRY(side_entry_ok(c, rgba8 || rgba_f64, nullptr, nullptr));
  OrthoView V;
  if (axis1 < 0 || axis1 > 2 || axis2 < 0 || axis2 > 2) return fail(RT_ERR_INVALID, "Invalid axes");
  if (axis1 != 0 && axis2 != 0) V.axis3 = 0;
  else if (axis1 != 1 && axis2 != 1) V.axis3 = 1;
  else if (axis1 != 2 && axis2 != 2) V.axis3 = 2;
  else return fail(RT_ERR_INVALID, "Invalid axes");                      // the reference panics
  V.axis1 = axis1; V.axis2 = axis2; V.dir1 = dir1; V.dir2 = dir2; V.scale = scale;
  if (y0 > y1 || y1 > (uint32_t)c->dev.height) return fail(RT_ERR_INVALID, "bad row range [%u, %u)", y0, y1);
  if (y0 == y1) return RT_OK;
  const int W = c->dev.width;
  const uint32_t n = y1 - y0;
  const size_t row4 = (size_t)W * 4, row32 = (size_t)W * 32;
  if (rgba8 && row_stride_bytes < row4) return fail(RT_ERR_INVALID, "row stride %zu < %zu", row_stride_bytes, row4);
  if (rgba_f64 && f64_stride < row32) return fail(RT_ERR_INVALID, "f64 stride %zu < %zu", f64_stride, row32);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  Stager sg;
  const int i8 = sg.add_out(rgba8, row_stride_bytes, row4, n, 0, "output");
  const int i_f = sg.add_out(rgba_f64, f64_stride, row32, n, 0, "f64");
  RT_TRY(sg.reserve(c, st));
  const int tiles = ((W + 15) / 16) * (int)((n + 15) / 16);
  RT_TRY(begin_launch(c, st));
  hipLaunchKernelGGL(ortho_kernel, dim3(tiles), dim3(256), 0, st, c->dev, V, (int)y0, (int)n, sg.ptr(i8), sg.stride(i8),
                     sg.ptr<double>(i_f), sg.stride(i_f));
  RT_TRY(end_launch(c, st));
  return sg.finish(st, false);
}

}  // extern "C"
