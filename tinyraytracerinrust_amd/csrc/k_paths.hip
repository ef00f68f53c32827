// k_paths.hip -- the ray debugger's recording (RayDebugger::record_rays, ray_debugger.rs:92-137, over the
// RayDebuggerCallback of raytracer.rs:17-19): of one sample (rt_record_rays: one thread, room for the whole ray tree) and of
// many in one launch (rt_ray_paths_offsets, rt_ray_paths): one lane per sample, every sample's records packed into a
// segment of exactly its size, in the reference's callback order.
//   count   paths_count_kernel: trace() with a recorder of one counter -> uint32 per sample;
//   scan    scan_*_kernel: the counts' exclusive prefix sum into uint64 offsets (paths_plan.h: three steps, no
//           workgroup waits for another);
//   fill    paths_fill_kernel: trace() with BufRec on the sample's segment of a scratch table -- records in START
//           order, the order table in callback order, made absolute;
//   gather  paths_gather_kernel: out[j] = tmp[order[j]] in 16-byte chunks, so the output is written coalesced.
// The fill's scratch is (160 + 4) bytes per record on top of the caller's output.  Memory safety never depends on the
// caller's offsets: a segment is cut to the buffer (path_segment), BufRec drops what does not fit, the order table
// starts as all ones and the gather skips every entry that is no index into the scratch.
#include "rt_device.h"
#include "rt_ctx.h"
#include "paths_plan.h"

namespace {

// The counting recorder: one ray per get_ray_color call (primary + reflect + refract: the records
// RayDebugger::record_rays would push).  finish() is empty, so trace()'s slot bookkeeping is dead.
struct PathCountRec {
  uint32_t n;
  __device__ __forceinline__ int begin(int, int, V3, V3, double, int, V3) { ++n; return 0; }
  __device__ __forceinline__ void finish(int, Col) {}
};

// One lane per sample, as render_points_kernel: the frame stack in the private array, no LDS.  No waves-per-SIMD
// pin: the row kernels' pins trade registers against their LDS frames and there are none here (DESIGN.md section 6
// "Ray paths" has the register counts).
template <bool REFR>
__global__ __launch_bounds__(256) void paths_count_kernel(RtDevScene S, const double* __restrict__ xy, uint32_t n,
                                                          int max_depth, uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 ro, rd;
  camera_ray(S.cam, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], &ro, &rd);
  PathCountRec R = {0u};
  (void)trace<REFR, PathCountRec>(make_ds(S), ro, rd, max_depth, &R);
  counts[i] = R.n;                                                       // one coalesced 4-byte store per lane
}

// Exclusive scan of one value per thread over a workgroup of RT_SCAN_THREADS (four waves): shuffles inside a wave,
// the waves' totals through LDS.  *total = the workgroup's sum.  Every thread of the workgroup calls it.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* total) {
  __shared__ T wave_sum[rt::RT_SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  T base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < (int)(rt::RT_SCAN_THREADS / 64); ++k) {
    if (k < wave) base += wave_sum[k];
    all += wave_sum[k];
  }
  __syncthreads();                                                       // the table is written again by the next call
  *total = all;
  return base + incl - v;
}

// Step 1: block b's sum of its RT_SCAN_BLOCK counts (a count is < 2^17 rays, so a block's sum fits 32 bits).
__global__ __launch_bounds__(rt::RT_SCAN_THREADS) void scan_sums_kernel(const uint32_t* __restrict__ counts, uint32_t n,
                                                                        unsigned long long* __restrict__ sums) {
  const uint32_t i0 = blockIdx.x * rt::RT_SCAN_BLOCK + threadIdx.x * rt::RT_SCAN_ITEMS;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < rt::RT_SCAN_ITEMS; ++k)
    if (i0 + k < n) v += counts[i0 + k];
  uint32_t total;
  (void)block_excl_scan<uint32_t>(v, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Step 2: ONE workgroup scans the nb block sums in place, RT_SCAN_BLOCK per round with the running total carried
// (the loop bounds are uniform over the workgroup), and appends the grand total at sums[nb].
__global__ __launch_bounds__(rt::RT_SCAN_THREADS) void scan_top_kernel(unsigned long long* __restrict__ sums, uint32_t nb) {
  unsigned long long carry = 0;
  for (uint32_t r0 = 0; r0 < nb; r0 += rt::RT_SCAN_BLOCK) {
    const uint32_t i0 = r0 + threadIdx.x * rt::RT_SCAN_ITEMS;
    unsigned long long e[rt::RT_SCAN_ITEMS], v = 0;
#pragma unroll
    for (uint32_t k = 0; k < rt::RT_SCAN_ITEMS; ++k) {
      e[k] = i0 + k < nb ? sums[i0 + k] : 0ull;
      v += e[k];
    }
    unsigned long long total;
    unsigned long long at = carry + block_excl_scan<unsigned long long>(v, &total);
#pragma unroll
    for (uint32_t k = 0; k < rt::RT_SCAN_ITEMS; ++k) {
      if (i0 + k < nb) sums[i0 + k] = at;                                 // each element is read and written by one thread
      at += e[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

// Step 3: block b's own exclusive scan plus its scanned sum (sums null: the single-workgroup path, base 0) ->
// offsets[i]; the last block appends offsets[n] = the total.
__global__ __launch_bounds__(rt::RT_SCAN_THREADS) void scan_write_kernel(const uint32_t* __restrict__ counts, uint32_t n,
                                                                         const unsigned long long* __restrict__ sums,
                                                                         unsigned long long* __restrict__ offsets) {
  const uint32_t i0 = blockIdx.x * rt::RT_SCAN_BLOCK + threadIdx.x * rt::RT_SCAN_ITEMS;
  uint32_t e[rt::RT_SCAN_ITEMS], v = 0;
#pragma unroll
  for (uint32_t k = 0; k < rt::RT_SCAN_ITEMS; ++k) {
    e[k] = i0 + k < n ? counts[i0 + k] : 0u;
    v += e[k];
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<uint32_t>(v, &total);
  const unsigned long long base = sums ? sums[blockIdx.x] : 0ull;
  unsigned long long at = base + excl;
#pragma unroll
  for (uint32_t k = 0; k < rt::RT_SCAN_ITEMS; ++k) {
    if (i0 + k < n) offsets[i0 + k] = at;
    at += e[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) offsets[n] = base + total;
}

// The status block the fill adds to, only on a mismatch: [0] samples whose segment is not their ray count,
// [1] records dropped because a segment was too short.
constexpr int PATHS_STATUS_WORDS = 2;

// One lane per sample: BufRec (rt_trace.h; the recorder of rt_record_rays, so the record contents are its) on the
// sample's segment of the scratch table -- `cap` records, every segment cut to it (path_segment).  The lane then
// makes its order entries absolute (the gather needs no search) and stores get_pixel's colour as
// render_points_kernel does.  Order entries the lane does not write keep the table's initial all-ones.
template <bool REFR>
__global__ __launch_bounds__(256) void paths_fill_kernel(RtDevScene S, const double* __restrict__ xy, uint32_t n,
                                                         int max_depth, const unsigned long long* __restrict__ offsets,
                                                         unsigned long long cap, RtRayRecord* __restrict__ tmp,
                                                         uint32_t* __restrict__ order, double* __restrict__ rgba,
                                                         uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const rt::PathSegment seg = rt::path_segment(offsets[i], offsets[i + 1], cap);
  const DS D = make_ds(S);
  BufRec R{tmp + seg.begin, (int*)(order + seg.begin), (int)seg.len, 0, 0, &D};
  V3 ro, rd;
  camera_ray(S.cam, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], &ro, &rd);
  const Col c = trace<REFR, BufRec>(D, ro, rd, max_depth, &R);
  const uint32_t done = (uint32_t)R.n_done < seg.len ? (uint32_t)R.n_done : seg.len;
  for (uint32_t j = 0; j < done; ++j) order[seg.begin + j] += (uint32_t)seg.begin;
  if (rgba) {
    double* o = rgba + 4 * (size_t)i;
    o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = 1.0;
  }
  const uint32_t begun = (uint32_t)R.n_begun;
  if (begun != seg.len) {
    atomicAdd(status, 1u);
    if (begun > seg.len) atomicAdd(status + 1, begun - seg.len);
  }
}

// rt_record_rays: one thread, the same recorder on a table that holds the whole ray tree; get_pixel's colour behind it.
template <bool REFR>
__global__ void record_ray_kernel(RtDevScene S, double x, double y, int max_depth, RtRayRecord* rec, int* order,
                                  int cap, int* counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const DS D = make_ds(S);
  BufRec R{rec, order, cap, 0, 0, &D};
  V3 ro, rd;
  camera_ray(S.cam, x, y, &ro, &rd);
  const Col c = trace<REFR, BufRec>(D, ro, rd, max_depth, &R);
  counts[0] = R.n_begun;
  counts[1] = R.n_done;
  rec[cap].color[0] = c.r; rec[cap].color[1] = c.g; rec[cap].color[2] = c.b; rec[cap].color[3] = 1.0;   // get_pixel's return
}

// One thread per (record, 16-byte chunk), ten chunks per 160-byte record: out[j] = tmp[order[j]].  Consecutive
// threads write consecutive 16 bytes.  An entry that is no index into the scratch (never written: its sample's
// rays did not fill the segment) leaves the output record alone.  Chunk 1 holds rt_ray_record::pad, which no
// recorder writes: stored as 0, so equal calls give equal bytes.
static_assert(sizeof(RtRayRecord) == 160, "the gather moves ten 16-byte chunks per record");
__global__ __launch_bounds__(256) void paths_gather_kernel(const uint4* __restrict__ tmp, const uint32_t* __restrict__ order,
                                                           unsigned long long m, uint4* __restrict__ out) {
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * 10ull) return;
  const unsigned long long j = t / 10ull;
  const uint32_t k = (uint32_t)(t - j * 10ull);
  const uint32_t o = order[j];
  if ((unsigned long long)o >= m) return;
  uint4 v = tmp[(unsigned long long)o * 10ull + k];
  if (k == 1) v.y = 0u;
  out[t] = v;
}

}  // namespace

using namespace rt;

// What both batched calls check first, in this order: the side entries' refusals for a perspective scene, the sample count.
static int paths_args_ok(rt_ctx* c, const char* who, const double* xy, size_t n, int32_t* max_depth, ScanPlan* plan) {
  RT_TRY(side_entry_ok(c, true, who, max_depth));
  *plan = plan_scan(n);
  if (plan->status == ScanPlan::TOO_MANY)
    return fail(RT_ERR_UNSUPPORTED, "%zu sample positions > %llu", n, (unsigned long long)RT_SCAN_MAX_N);
  if (n > 0 && !xy) return fail(RT_ERR_INVALID, "null argument");
  return RT_OK;
}

extern "C" {

int rt_ray_paths_offsets(rt_ctx* c, const double* xy, size_t n, int32_t max_depth, uint64_t* offsets, uint64_t* total,
                         void* stream) {
  if (!offsets) return fail(RT_ERR_INVALID, "null argument");
  ScanPlan plan;
  RT_TRY(paths_args_ok(c, "rt_ray_paths_offsets", xy, n, &max_depth, &plan));
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  if (plan.status == ScanPlan::NOTHING) {
    if (is_device_ptr(offsets)) RT_HIP(hipMemsetAsync(offsets, 0, 8, st));
    else offsets[0] = 0;
    if (total) {
      RT_HIP(hipStreamSynchronize(st));
      *total = 0;
    }
    return RT_OK;
  }
  Stager sg;
  const int i_xy = sg.add_in(xy, n * 16, n * 16, 1, 8, "sample position");
  const int i_off = sg.add_out(offsets, (n + 1) * 8, (n + 1) * 8, 1, 8, "offset");
  const int i_cnt = sg.add_scratch(n * 4), i_sums = sg.add_scratch(plan.two_level ? (size_t)plan.sums_bytes : 8);
  RT_TRY(sg.reserve(c, st));
  const double* in = sg.ptr<const double>(i_xy);
  unsigned long long* k_off = sg.ptr<unsigned long long>(i_off);
  uint32_t* k_cnt = sg.ptr<uint32_t>(i_cnt);
  unsigned long long* k_sums = plan.two_level ? sg.ptr<unsigned long long>(i_sums) : nullptr;
  const uint32_t n32 = (uint32_t)n;
  const dim3 grid((n32 + 255) / 256), block(256), sgrid(plan.n_blocks), sblock(RT_SCAN_THREADS);
  RT_TRY(begin_launch(c, st));
  with_bool(c->dev.any_transparent != 0, [&](auto R) {
    hipLaunchKernelGGL((paths_count_kernel<decltype(R)::value>), grid, block, 0, st, c->dev, in, n32, (int)max_depth, k_cnt);
  });
  if (plan.two_level) {
    hipLaunchKernelGGL(scan_sums_kernel, sgrid, sblock, 0, st, k_cnt, n32, k_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), sblock, 0, st, k_sums, plan.n_blocks);
  }
  hipLaunchKernelGGL(scan_write_kernel, sgrid, sblock, 0, st, k_cnt, n32, k_sums, k_off);
  RT_TRY(end_launch(c, st));
  uint64_t sum = 0;
  if (total) RT_HIP(hipMemcpyAsync(&sum, k_off + n, 8, hipMemcpyDeviceToHost, st));
  RT_TRY(sg.finish(st, total != nullptr));
  if (total) *total = sum;
  return RT_OK;
}

int rt_ray_paths(rt_ctx* c, const double* xy, size_t n, int32_t max_depth, const uint64_t* offsets, rt_ray_record* records,
                 size_t cap_records, double* rgba_f64, void* stream) {
  ScanPlan plan;
  RT_TRY(paths_args_ok(c, "rt_ray_paths", xy, n, &max_depth, &plan));
  if (plan.status == ScanPlan::NOTHING) return RT_OK;
  if (!offsets || (!records && cap_records > 0)) return fail(RT_ERR_INVALID, "null argument");
  RT_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;   // NULL = the device's default stream
  // the records the call can touch: the caller's buffer cut to what the offsets claim, offsets[n] -- read here, once,
  // to size the scratch (behind whatever produced the offsets on st)
  uint64_t claimed = 0;
  if (is_device_ptr(offsets)) {
    RT_HIP(hipMemcpyAsync(&claimed, offsets + n, 8, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
  } else {
    claimed = offsets[n];
  }
  const uint64_t m = claimed < (uint64_t)cap_records ? claimed : (uint64_t)cap_records;
  if (m > RT_PATHS_MAX_RECORDS) return fail(RT_ERR_UNSUPPORTED, "%llu records > %llu", (unsigned long long)m, (unsigned long long)RT_PATHS_MAX_RECORDS);
  const size_t rec_bytes = (size_t)m * sizeof(rt_ray_record), ord_bytes = ((size_t)m * 4 + 255) & ~(size_t)255;
  Stager sg;
  const int i_xy = sg.add_in(xy, n * 16, n * 16, 1, 8, "sample position");
  const int i_off = sg.add_in(offsets, (n + 1) * 8, (n + 1) * 8, 1, 8, "offset");
  const int i_rec = sg.add_out(m ? records : nullptr, rec_bytes, rec_bytes, 1, 16, "record");
  const int i_rgba = sg.add_out(rgba_f64, n * 32, n * 32, 1, 8, "colour");
  const int i_tmp = sg.add_scratch(rec_bytes);
  const int i_tab = sg.add_scratch(ord_bytes + 256);                     // the order table, then the status block
  RT_TRY(sg.reserve(c, st));
  uint8_t* tab = sg.ptr(i_tab);
  uint32_t* k_order = (uint32_t*)tab;
  uint32_t* k_status = (uint32_t*)(tab + ord_bytes);
  // ahead of the timing event, as the count's sums (k_stats.hip): the order table all ones, the status zero
  if (m) RT_HIP(hipMemsetAsync(k_order, 0xff, (size_t)m * 4, st));
  RT_HIP(hipMemsetAsync(k_status, 0, 256, st));
  const uint32_t n32 = (uint32_t)n;
  const dim3 grid((n32 + 255) / 256), block(256);
  RT_TRY(begin_launch(c, st));
  with_bool(c->dev.any_transparent != 0, [&](auto R) {
    hipLaunchKernelGGL((paths_fill_kernel<decltype(R)::value>), grid, block, 0, st, c->dev, sg.ptr<const double>(i_xy), n32,
                       (int)max_depth, sg.ptr<const unsigned long long>(i_off), (unsigned long long)m,
                       sg.ptr<RtRayRecord>(i_tmp), k_order, sg.ptr<double>(i_rgba), k_status);
  });
  if (m) {
    const dim3 ggrid((unsigned)((m * 10 + 255) / 256));
    hipLaunchKernelGGL(paths_gather_kernel, ggrid, block, 0, st, sg.ptr<const uint4>(i_tmp), k_order, (unsigned long long)m,
                       sg.ptr<uint4>(i_rec));
  }
  RT_TRY(end_launch(c, st));
  uint32_t status[PATHS_STATUS_WORDS] = {0, 0};
  RT_HIP(hipMemcpyAsync(status, k_status, sizeof status, hipMemcpyDeviceToHost, st));
  RT_TRY(sg.finish(st, true));
  if (status[0])
    return fail(RT_ERR_INVALID, "%u of %zu samples trace another number of rays than their offsets say (%u records dropped): "
                "stale offsets, another depth or scene, or cap_records below offsets[n]", status[0], n, status[1]);
  return RT_OK;
}

// RayDebugger::record_rays (ray_debugger.rs:92-137): one thread, records in callback order.
int rt_record_rays(rt_ctx* c, double x, double y, int32_t max_depth, rt_ray_record* records, int32_t cap,
                   int32_t* n_rays, double* rgba) {
  RT_TRY(side_entry_ok(c, (records || cap <= 0) && cap >= 0 && n_rays, "rt_record_rays", &max_depth));
  RT_HIP(hipSetDevice(c->device));
  // room for the whole ray tree: a chain of max_depth + 1 rays, or a binary tree with refraction
  const bool refr = c->dev.any_transparent != 0;
  const int dev_cap = refr ? (2 << max_depth) - 1 : max_depth + 1;
  const size_t rec_bytes = sizeof(rt_ray_record) * ((size_t)dev_cap + 1);
  hipStream_t st = nullptr;
  Stager sg;                                // the recorder's tables: records, their callback order, two counters
  const int i_rec = sg.add_scratch(rec_bytes), i_ord = sg.add_scratch((size_t)dev_cap * 4), i_cnt = sg.add_scratch(64);
  RT_TRY(sg.reserve(c, st));
  rt_ray_record* d_rec = sg.ptr<rt_ray_record>(i_rec);
  int* d_ord = sg.ptr<int>(i_ord);
  int* d_cnt = sg.ptr<int>(i_cnt);
  with_bool(refr, [&](auto R) {
    hipLaunchKernelGGL((record_ray_kernel<decltype(R)::value>), dim3(1), dim3(64), 0, st, c->dev, x, y, (int)max_depth, d_rec,
                       d_ord, dev_cap, d_cnt);
  });
  RT_HIP(hipGetLastError());
  RT_TRY(rt::mark_launch(c, st));
  int cnt[2] = {0, 0};
  RT_HIP(hipMemcpy(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
  if (cnt[0] != cnt[1] || cnt[1] > dev_cap) return fail(RT_ERR_DEVICE, "ray recorder overflow (%d/%d of %d)", cnt[0], cnt[1], dev_cap);
  std::vector<rt_ray_record> rec((size_t)dev_cap + 1);
  std::vector<int> ord((size_t)dev_cap);
  RT_HIP(hipMemcpy(rec.data(), d_rec, rec_bytes, hipMemcpyDeviceToHost));
  RT_HIP(hipMemcpy(ord.data(), d_ord, sizeof(int) * (size_t)dev_cap, hipMemcpyDeviceToHost));
  *n_rays = cnt[1];
  const int keep = cnt[1] < cap ? cnt[1] : cap;
  for (int i = 0; i < keep; ++i) records[i] = rec[(size_t)ord[i]];
  if (rgba) for (int k = 0; k < 4; ++k) rgba[k] = rec[(size_t)dev_cap].color[k];
  return RT_OK;
}

}  // extern "C"
