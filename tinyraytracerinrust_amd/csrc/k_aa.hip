// k_aa.hip -- the adaptive anti-aliasing pass (rt_antialias, rt_antialias_row_bands; antialiaser.rs:87-191) and its
// edge overlay (rt_antialias_edges; :173-191), behind the same C ABI as the row loop.  What the pass allocates for its
// edge pixels is aa_plan.h's (pure host code); this unit carries it out.
#include "rt_device.h"
#include "rt_ctx.h"
#include "aa_plan.h"

namespace {

// antialiaser.rs:87-191 as driven by debug_window.rs:275-320, breadth-first instead of the
// reference's depth-first memoised recursion (same decisions, same traced sub-pixel set, same
// arithmetic):
//   aa_classify  one thread per pixel: the root cell's corners come from the QUANTISED frame
//                (u8 / 255); non-edge pixels are finished here, edge pixels are compacted into a
//                list with one ballot + one atomic per wave;
//   aa_expand    pass p = 1..level, one thread per edge pixel: walk the cell tree to depth p-1,
//                every cell there that subdivides requests its five new grid points (the per-pixel
//                have-mask is the reference's Option<Color> memo);
//   aa_trace     one thread per requested sub-pixel: get_pixel(x + sx/size, y + sy/size);
//   aa_resolve   one thread per edge pixel: the reference recursion over the filled grid.
// Grid points are [sx][sy] as sub_pixels[sub_x][sub_y] (antialiaser.rs:96-99).
struct AaCol { double r, g, b, a; };
static_assert(sizeof(AaCol) == rt::RT_AA_COL_BYTES && sizeof(uint2) == rt::RT_AA_REQ_BYTES, "aa_plan.h lays these out");

__device__ __forceinline__ AaCol aa_src(const uint8_t* src, size_t stride, int x, int y) {   // easy_pixbuf.rs:55-64
  const uint8_t* p = src + (size_t)y * stride + (size_t)x * 4;
  return {p[0] / 255.0, p[1] / 255.0, p[2] / 255.0, p[3] / 255.0};
}
__device__ __forceinline__ bool aa_diff(AaCol c1, AaCol c2, double th) {                   // :154-162
  return (fabs(c1.r - c2.r) + fabs(c1.g - c2.g) + fabs(c1.b - c2.b) + fabs(c1.a - c2.a)) / 4.0 > th;
}
// A cell's first corner against its three others: the cell subdivides, the pixel is an edge (:124-131, :173-191)
__device__ __forceinline__ bool aa_corners_differ(AaCol c1, AaCol c2, AaCol c3, AaCol c4, double th) {
  return aa_diff(c1, c2, th) || aa_diff(c1, c3, th) || aa_diff(c1, c4, th);
}
__device__ __forceinline__ AaCol aa_avg(AaCol c1, AaCol c2, AaCol c3, AaCol c4) {           // :164-171
  return {(c1.r + c2.r + c3.r + c4.r) / 4.0, (c1.g + c2.g + c3.g + c4.g) / 4.0,
          (c1.b + c2.b + c3.b + c4.b) / 4.0, (c1.a + c2.a + c3.a + c4.a) / 4.0};
}
__device__ __forceinline__ void aa_put(AaCol c, int x, int y, uint8_t* u8, size_t u8_stride, double* f64, size_t f64_stride) {
  put_rgba(c.r, c.g, c.b, c.a, x, y, u8, u8_stride, f64, f64_stride);
}

struct AaGrid {             // per edge pixel: size*size colours + have bits
  AaCol* col;
  uint64_t* have;           // RT_AA_HAVE_WORDS words per edge pixel
  int size;
};

// The rows a call owns: rt_render_row_bands' geometry (rt_device.h band_row).  The source is always the whole
// frame; the OUTPUT holds the owned rows packed, n_rows of them (the host has dropped the rows >= H, which can
// only be the layout's last).  The whole frame is the one band (0, H, H, H): a wave-uniform branch, no division.
struct AaBands { int y_first, band_rows, band_pitch, n_rows; };

__device__ __forceinline__ int aa_packed_row(const AaBands& B, int y) {   // band_row's inverse, for an owned row
  const int d = y - B.y_first;
  if (B.band_rows >= B.n_rows) return d;
  return (d / B.band_pitch) * B.band_rows + d % B.band_pitch;
}

// 16x16 tiles over (W, packed rows): tiles straddle bands when band_rows is no multiple of 8; the edge list
// keeps FRAME coordinates, so only this kernel's and aa_resolve's stores know about packing.
__global__ __launch_bounds__(256) void aa_classify_kernel(const uint8_t* __restrict__ src, size_t stride, int W, int H,
                                                          AaBands B, double th, int level, uint8_t* u8, size_t u8_stride,
                                                          double* f64, size_t f64_stride, uint32_t* __restrict__ edges,
                                                          uint32_t* __restrict__ n_edges) {
  const int lane = threadIdx.x & 63;
  int x, r;
  tile16_pixel(blockIdx.x, threadIdx.x, W, &x, &r);
  const int y = band_row(r, B.y_first, B.band_rows, B.band_pitch, B.n_rows);
  bool edge = false;
  if (x < W && r < B.n_rows) {               // every packed row below n_rows is a frame row (the host drops the others)
    if (x == W - 1 || y == H - 1) {          // last column copied (:67-68); last row never touched (debug_window.rs:298)
      aa_put(aa_src(src, stride, x, y), x, r, u8, u8_stride, f64, f64_stride);
    } else {
      const AaCol c1 = aa_src(src, stride, x, y), c2 = aa_src(src, stride, x + 1, y);
      const AaCol c3 = aa_src(src, stride, x, y + 1), c4 = aa_src(src, stride, x + 1, y + 1);
      edge = level > 0 && aa_corners_differ(c1, c2, c3, c4, th);
      if (!edge) aa_put(aa_avg(c1, c2, c3, c4), x, r, u8, u8_stride, f64, f64_stride);
    }
  }
  const uint64_t m = __ballot(edge);                                   // wave-aggregated compaction
  if (m == 0) return;
  uint32_t base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(n_edges, (uint32_t)__popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (edge) edges[base + __popcll(m & ((1ull << lane) - 1))] = ((uint32_t)y << 16) | (uint32_t)x;
}

// AntiAliaser::mark_edge_pixels (:173-191) as check_anti_aliasing_threshold paints it (debug_window.rs:116-139):
// the classify kernel's corner predicate without its level term, over the whole frame.  One thread per pixel
// writes `mark` or Color::EMPTY; one ballot + one atomic per wave counts the marks.
__global__ __launch_bounds__(256) void aa_edges_kernel(const uint8_t* __restrict__ src, size_t stride, int W, int H,
                                                       double th, uint8_t* __restrict__ out, size_t out_stride,
                                                       uint32_t* __restrict__ n_marked) {
  const uint32_t mark = to_u8(0.6) | (to_u8(1.0) << 8) | (to_u8(1.0) << 16) | (to_u8(0.5) << 24);   // debug_window.rs:130
  const int lane = threadIdx.x & 63;
  int x, y;
  tile16_pixel(blockIdx.x, threadIdx.x, W, &x, &y);
  bool edge = false;
  if (x < W && y < H) {
    if (x < W - 1 && y < H - 1)
      edge = aa_corners_differ(aa_src(src, stride, x, y), aa_src(src, stride, x, y + 1), aa_src(src, stride, x + 1, y),
                               aa_src(src, stride, x + 1, y + 1), th);
    ((uint32_t*)(out + (size_t)y * out_stride))[x] = edge ? mark : 0u;
  }
  const uint64_t m = __ballot(edge);
  if (m != 0 && lane == __ffsll((long long)m) - 1) atomicAdd(n_marked, (uint32_t)__popcll(m));
}

__device__ __forceinline__ bool aa_has(const uint64_t* h, int i) { return (h[i >> 6] >> (i & 63)) & 1u; }

// Depth-first walk to depth `target`; cells there that subdivide request their new points
// (have = the pixel's memo bits, updated).  With req == nullptr only counts; otherwise writes the
// requests to req[base ...].  Returns the number of new points.
__device__ uint32_t aa_expand_cell(const AaGrid& G, uint32_t e, int target, int level, double th, uint64_t* have,
                                   uint2* req, uint32_t base) {
  struct Frame { int8_t x1, y1, x2, y2, depth; };
  Frame st[4 * RT_AA_MAX_LEVEL + 4];
  int sp = 0;
  const int sz = G.size;
  st[sp++] = {0, 0, (int8_t)(sz - 1), (int8_t)(sz - 1), 0};
  const AaCol* col = G.col + (size_t)e * sz * sz;
  uint32_t n = 0;
  while (sp > 0) {
    const Frame f = st[--sp];
    const AaCol c1 = col[f.x1 * sz + f.y1], c2 = col[f.x2 * sz + f.y1];
    const AaCol c3 = col[f.x1 * sz + f.y2], c4 = col[f.x2 * sz + f.y2];
    const bool split = (level - f.depth) > 0 && aa_corners_differ(c1, c2, c3, c4, th);
    if (!split) continue;
    const int mx = f.x1 + (f.x2 - f.x1) / 2, my = f.y1 + (f.y2 - f.y1) / 2;
    if (f.depth < target) {                                    // children, pushed so the first pops first
      st[sp++] = {(int8_t)mx, (int8_t)my, f.x2, f.y2, (int8_t)(f.depth + 1)};
      st[sp++] = {f.x1, (int8_t)my, (int8_t)mx, f.y2, (int8_t)(f.depth + 1)};
      st[sp++] = {(int8_t)mx, f.y1, f.x2, (int8_t)my, (int8_t)(f.depth + 1)};
      st[sp++] = {f.x1, f.y1, (int8_t)mx, (int8_t)my, (int8_t)(f.depth + 1)};
      continue;
    }
    const int px[5] = {mx, f.x1, mx, f.x2, mx}, py[5] = {f.y1, my, my, my, f.y2};
    for (int k = 0; k < 5; ++k) {
      const int i = px[k] * sz + py[k];
      if (aa_has(have, i)) continue;
      have[i >> 6] |= 1ull << (i & 63);
      if (req) req[base + n] = make_uint2(e, (uint32_t)(px[k] | (py[k] << 8)));
      ++n;
    }
  }
  return n;
}

__global__ __launch_bounds__(256) void aa_init_kernel(AaGrid G, const uint8_t* __restrict__ src, size_t stride,
                                                      const uint32_t* __restrict__ edges, uint32_t n) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int x = edges[e] & 0xffff, y = edges[e] >> 16, sz = G.size, nn = sz - 1;
  AaCol* col = G.col + (size_t)e * sz * sz;
  uint64_t* h = G.have + (size_t)e * RT_AA_HAVE_WORDS;
  for (int w = 0; w < RT_AA_HAVE_WORDS; ++w) h[w] = 0;
  const int idx[4] = {0, nn, nn * sz, nn * sz + nn};                  // [0][0] [0][n] [n][0] [n][n] (:96-99)
  col[idx[0]] = aa_src(src, stride, x, y);
  col[idx[1]] = aa_src(src, stride, x, y + 1);
  col[idx[2]] = aa_src(src, stride, x + 1, y);
  col[idx[3]] = aa_src(src, stride, x + 1, y + 1);
  for (int k = 0; k < 4; ++k) h[idx[k] >> 6] |= 1ull << (idx[k] & 63);
}

__global__ __launch_bounds__(256) void aa_expand_kernel(AaGrid G, uint32_t n, int pass, int level, double th,
                                                        uint2* __restrict__ req, uint32_t* __restrict__ n_req,
                                                        uint32_t cap) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < n;
  uint64_t have[RT_AA_HAVE_WORDS], probe[RT_AA_HAVE_WORDS];
  uint32_t cnt = 0;
  if (live) {
    const uint64_t* h = G.have + (size_t)e * RT_AA_HAVE_WORDS;
    for (int w = 0; w < RT_AA_HAVE_WORDS; ++w) probe[w] = have[w] = h[w];
    cnt = aa_expand_cell(G, e, pass - 1, level, th, probe, nullptr, 0);   // count
  }
  // one atomic per wave: exclusive prefix of the lane counts
  const int lane = threadIdx.x & 63;
  uint32_t incl = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  const uint32_t total = __shfl(incl, 63);
  uint32_t base = 0;
  if (lane == 63 && total > 0) base = atomicAdd(n_req, total);
  base = __shfl(base, 63) + (incl - cnt);
  if (!live || cnt == 0) return;
  if (base + cnt > cap) return;                                          // host reports the overflow
  aa_expand_cell(G, e, pass - 1, level, th, have, req, base);            // write
  uint64_t* h = G.have + (size_t)e * RT_AA_HAVE_WORDS;
  for (int w = 0; w < RT_AA_HAVE_WORDS; ++w) h[w] = have[w];
}

// One-wave workgroups with the frame stack's first frames in LDS, as the row kernels.
template <bool REFR, bool FC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WAVES(REFR)))) void aa_trace_kernel(
    RtDevScene S, AaGrid G, const uint32_t* __restrict__ edges, const uint2* __restrict__ req, uint32_t n, int max_depth) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  constexpr int KLR = REFR ? RT_LDS_RFRAMES : 0;
  __shared__ double s_frames[(RT_LDS_FRAMES * 4 + KLR * 7) * 64 + 1];
  lds_f64* lf = (lds_f64*)&s_frames[threadIdx.x];
  if (i >= n) return;
  const uint2 r = req[i];
  const int x = edges[r.x] & 0xffff, y = edges[r.x] >> 16;
  const int sx = r.y & 0xff, sy = r.y >> 8, sz = G.size;
  V3 ro, rd;
  camera_ray(S.cam, (double)x + ((double)sx / (double)sz), (double)y + ((double)sy / (double)sz), &ro, &rd);   // :108-112
  const Col c = trace<REFR, NoRec, RT_LDS_FRAMES, FC, KLR>(make_ds(S), ro, rd, max_depth, nullptr, lf);
  G.col[(size_t)r.x * sz * sz + sx * sz + sy] = {c.r, c.g, c.b, 1.0};
}

// get_sub_pixel_color (:124-152) over the filled grid; D bounds the remaining depth at compile time.
// Fully inlined (256 VGPRs, no scratch): measured faster than an explicit-stack loop, whose frame
// array lives in scratch (profiles/r01j_aa_timing.txt).  The corner predicate stays written out here: through
// aa_corners_differ the recursion is inlined another way (230 VGPRs, untimed; profiles/r26a_side_split.txt).
template <int D>
__device__ AaCol aa_cell(const AaCol* col, int sz, int x1, int y1, int x2, int y2, int lv, double th) {
  const AaCol c1 = col[x1 * sz + y1], c2 = col[x2 * sz + y1], c3 = col[x1 * sz + y2], c4 = col[x2 * sz + y2];
  if constexpr (D == 0) {
    return aa_avg(c1, c2, c3, c4);
  } else {
    if (!(aa_diff(c1, c2, th) || aa_diff(c1, c3, th) || aa_diff(c1, c4, th)) || lv <= 0) return aa_avg(c1, c2, c3, c4);
    const int mx = x1 + (x2 - x1) / 2, my = y1 + (y2 - y1) / 2;
    const AaCol k1 = aa_cell<D - 1>(col, sz, x1, y1, mx, my, lv - 1, th);
    const AaCol k2 = aa_cell<D - 1>(col, sz, mx, y1, x2, my, lv - 1, th);
    const AaCol k3 = aa_cell<D - 1>(col, sz, x1, my, mx, y2, lv - 1, th);
    const AaCol k4 = aa_cell<D - 1>(col, sz, mx, my, x2, y2, lv - 1, th);
    return aa_avg(k1, k2, k3, k4);
  }
}

__global__ __launch_bounds__(256) void aa_resolve_kernel(AaGrid G, const uint32_t* __restrict__ edges, uint32_t n,
                                                         int level, double th, AaBands B, uint8_t* u8,
                                                         size_t u8_stride, double* f64, size_t f64_stride) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int sz = G.size;
  const AaCol* col = G.col + (size_t)e * sz * sz;
  const AaCol res = aa_cell<RT_AA_MAX_LEVEL>(col, sz, 0, 0, sz - 1, sz - 1, level, th);
  aa_put(res, edges[e] & 0xffff, aa_packed_row(B, edges[e] >> 16), u8, u8_stride, f64, f64_stride);
}

struct AaWork {   // the edge pixels' work block (aa_plan.h lays it out): freed on the call's stream however the call ends
  hipStream_t st;
  uint8_t* p = nullptr;
  ~AaWork() { if (p) (void)hipFreeAsync(p, st); }
};

}  // namespace

using namespace rt;

// antialiaser.rs:87-191 over the rows of a band layout of a whole quantised frame (see the kernels above):
// rt_antialias passes one band of more rows than any frame has, which clamp_bands (launch_plan.h) makes the layout
// (0, H, H, 1); rt_antialias_row_bands passes its caller's.  `who` names the entry in the one error text that does.
static int antialias_rows(rt_ctx* c, const char* who, const uint8_t* src_rgba8, size_t src_stride, double threshold,
                          int32_t level, int32_t max_depth, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch,
                          uint32_t n_bands, uint8_t* dst_rgba8, size_t dst_stride, double* dst_f64,
                          size_t f64_stride, uint64_t* rays_traced, void* stream) {
  RT_TRY(side_entry_ok(c, src_rgba8 && (dst_rgba8 || dst_f64), who, nullptr));
  if (level < 0) level = 0;
  if (level > RT_AA_MAX_LEVEL) return fail(RT_ERR_UNSUPPORTED, "anti-aliasing level %d > %d", level, RT_AA_MAX_LEVEL);
  if (!(threshold == threshold)) return fail(RT_ERR_INVALID, "threshold is NaN");
  RT_TRY(side_depth_ok(c, &max_depth));
  const int W = c->dev.width, H = c->dev.height;
  if (W > 65535 || H > 65535) return fail(RT_ERR_UNSUPPORTED, "frame %dx%d too large for the edge list", W, H);
  const size_t row4 = (size_t)W * 4, row32 = (size_t)W * 32;
  if (src_stride < row4) return fail(RT_ERR_INVALID, "source stride %zu < %zu", src_stride, row4);
  if (dst_rgba8 && dst_stride < row4) return fail(RT_ERR_INVALID, "output stride %zu < %zu", dst_stride, row4);
  if (dst_f64 && f64_stride < row32) return fail(RT_ERR_INVALID, "f64 stride %zu < %zu", f64_stride, row32);
  const BandGeometry g = clamp_bands(W, H, y_first, band_rows, band_pitch, n_bands);   // n_rows packed rows that all exist
  if (g.status == BandGeometry::NOTHING) {
    if (rays_traced) *rays_traced = 0;
    return RT_OK;
  }
  if (g.status != BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  const AaBands B = {(int)g.y_first, (int)g.band_rows, (int)g.band_pitch, (int)g.n_rows};
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  // the trace passes' kernel: the scene's specialised one once it is loaded (requested here on the first call
  // after an upload, polled without blocking); last_sample names it only if a pass launches
  const char* const sample_before = c->spec.last_sample;
  const hipFunction_t sfn = spec_sample_kernel(c, SPEC_AA);
  const char* const sample_ran = c->spec.last_sample;
  c->spec.last_sample = sample_before;
  // the whole source frame and the call's output rows in place or staged; the edge list and the counters
  Stager sg;
  const int i_src = sg.add_in(src_rgba8, src_stride, row4, H, 0, "source");
  const int i_u8 = sg.add_out(dst_rgba8, dst_stride, row4, g.n_rows, 0, "output");
  const int i_f64 = sg.add_out(dst_f64, f64_stride, row32, g.n_rows, 0, "f64");
  const int i_edges = sg.add_scratch((size_t)W * g.n_rows * 4), i_cnt = sg.add_scratch(64);   // an entry per pixel of the call
  RT_TRY(sg.reserve(c, st));
  const uint8_t* src = sg.ptr(i_src);
  uint8_t* u8 = sg.ptr(i_u8);
  double* f64 = sg.ptr<double>(i_f64);
  const size_t sstride = sg.stride(i_src), u8s = sg.stride(i_u8), f64s = sg.stride(i_f64);
  uint32_t* edges = sg.ptr<uint32_t>(i_edges);
  uint32_t* cnt = sg.ptr<uint32_t>(i_cnt);
  RT_HIP(hipMemsetAsync(cnt, 0, 64, st));   // ahead of the timing event, as the count's sums (k_stats.hip)
  RT_TRY(begin_launch(c, st));
  const int tiles = ((W + 15) / 16) * (((int)g.n_rows + 15) / 16);
  hipLaunchKernelGGL(aa_classify_kernel, dim3(tiles), dim3(256), 0, st, src, sstride, W, H, B, threshold, (int)level,
                     u8, u8s, f64, f64s, edges, cnt);
  RT_HIP(hipGetLastError());
  uint32_t n_edges = 0;
  RT_HIP(hipMemcpyAsync(&n_edges, cnt, 4, hipMemcpyDeviceToHost, st));
  RT_HIP(hipStreamSynchronize(st));
  uint64_t rays = 0;
  const AaPlan plan = plan_aa(level, n_edges);
  if (plan.status == AaPlan::TOO_MANY) return fail(RT_ERR_UNSUPPORTED, "too many anti-aliasing samples");
  if (plan.status == AaPlan::OK) {
    AaWork work{st};
    RT_HIP(hipMallocAsync((void**)&work.p, plan.bytes, st));
    const AaGrid G = {(AaCol*)(work.p + plan.col_off), (uint64_t*)(work.p + plan.have_off), plan.size};
    uint2* req = (uint2*)(work.p + plan.req_off);
    const dim3 eg((n_edges + 255) / 256), blk(256);
    hipLaunchKernelGGL(aa_init_kernel, eg, blk, 0, st, G, src, sstride, edges, n_edges);
    for (int pass = 1; pass <= level; ++pass) {
      RT_HIP(hipMemsetAsync(cnt + 1, 0, 4, st));
      hipLaunchKernelGGL(aa_expand_kernel, eg, blk, 0, st, G, n_edges, pass, (int)level, threshold, req, cnt + 1, (uint32_t)plan.cap);
      uint32_t n_req = 0;
      RT_HIP(hipMemcpyAsync(&n_req, cnt + 1, 4, hipMemcpyDeviceToHost, st));
      RT_HIP(hipStreamSynchronize(st));
      if (n_req > plan.cap) return fail(RT_ERR_DEVICE, "anti-aliasing request overflow (%u > %zu)", n_req, plan.cap);
      if (n_req == 0) break;
      rays += n_req;
      const dim3 rg((n_req + 63) / 64);
      c->spec.last_sample = sample_ran;
      if (sfn) {                                                 // the scene's specialised trace kernel (the catalogue's rt_spec_aa)
        int depth = max_depth, size = plan.size;
        double* col = (double*)G.col;
        void* kargs[] = {&c->dev, (void*)&edges, (void*)&req, &n_req, &size, &col, &depth};
        RT_HIP(hipModuleLaunchKernel(sfn, rg.x, 1, 1, 64, 1, 1, 0, st, kargs, nullptr));
      } else {
        with_bool(c->dev.any_transparent != 0, [&](auto R) { with_bool(c->dev.colour_fast != 0 && c->fast_clamp, [&](auto F) {
          hipLaunchKernelGGL((aa_trace_kernel<decltype(R)::value, decltype(F)::value>), rg, dim3(64), 0, st, c->dev, G, edges,
                             req, n_req, (int)max_depth);
        }); });
      }
    }
    hipLaunchKernelGGL(aa_resolve_kernel, eg, blk, 0, st, G, edges, n_edges, (int)level, threshold, B, u8, u8s, f64, f64s);
    RT_HIP(hipGetLastError());
  }
  RT_TRY(end_launch(c, st));
  RT_TRY(sg.finish(st, true));              // (the call has waited for its edge count: it ends synchronous)
  if (rays_traced) *rays_traced = rays;
  return RT_OK;
}

extern "C" {

int rt_antialias(rt_ctx* c, const uint8_t* src_rgba8, size_t src_stride, double threshold, int32_t level,
                 int32_t max_depth, uint8_t* dst_rgba8, size_t dst_stride, double* dst_f64, size_t f64_stride,
                 uint64_t* rays_traced, void* stream) {
  return antialias_rows(c, "rt_antialias", src_rgba8, src_stride, threshold, level, max_depth, 0, UINT32_MAX, UINT32_MAX, 1,
                        dst_rgba8, dst_stride, dst_f64, f64_stride, rays_traced, stream);
}

int rt_antialias_row_bands(rt_ctx* c, const uint8_t* src_rgba8, size_t src_stride, double threshold, int32_t level,
                           int32_t max_depth, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                           uint8_t* dst_rgba8, size_t dst_stride, double* dst_f64, size_t f64_stride,
                           uint64_t* rays_traced, void* stream) {
  return antialias_rows(c, "rt_antialias_row_bands", src_rgba8, src_stride, threshold, level, max_depth, y_first, band_rows,
                        band_pitch, n_bands, dst_rgba8, dst_stride, dst_f64, f64_stride, rays_traced, stream);
}

// AntiAliaser::mark_edge_pixels (antialiaser.rs:173-191) into an overlay, as check_anti_aliasing_threshold
// (debug_window.rs:116-139) builds the GUI's "show edges" layer.
int rt_antialias_edges(rt_ctx* c, const uint8_t* src_rgba8, size_t src_stride, double threshold, uint8_t* overlay_rgba8,
                       size_t overlay_stride, uint32_t* n_edges, void* stream) {
  RT_TRY(side_entry_ok(c, src_rgba8 && overlay_rgba8, nullptr, nullptr));
  if (!(threshold == threshold)) return fail(RT_ERR_INVALID, "threshold is NaN");
  const int W = c->dev.width, H = c->dev.height;
  const size_t row4 = (size_t)W * 4;
  if (src_stride < row4) return fail(RT_ERR_INVALID, "source stride %zu < %zu", src_stride, row4);
  if (overlay_stride < row4) return fail(RT_ERR_INVALID, "overlay stride %zu < %zu", overlay_stride, row4);
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  Stager sg;
  const int i_out = sg.add_out(overlay_rgba8, overlay_stride, row4, H, 4, "overlay");
  const int i_src = sg.add_in(src_rgba8, src_stride, row4, H, 0, "source");
  const int i_cnt = sg.add_scratch(64);
  RT_TRY(sg.reserve(c, st));
  uint32_t* cnt = sg.ptr<uint32_t>(i_cnt);
  RT_HIP(hipMemsetAsync(cnt, 0, 64, st));
  const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
  hipLaunchKernelGGL(aa_edges_kernel, dim3(tiles), dim3(256), 0, st, sg.ptr<const uint8_t>(i_src), sg.stride(i_src), W, H, threshold,
                     sg.ptr(i_out), sg.stride(i_out), cnt);
  RT_HIP(hipGetLastError());
  RT_TRY(rt::mark_launch(c, st));           // (no timing pair: the overlay is no render)
  uint32_t n = 0;
  if (n_edges) RT_HIP(hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, st));
  RT_TRY(sg.finish(st, n_edges != nullptr));
  if (n_edges) *n_edges = n;
  return RT_OK;
}

}  // extern "C"
