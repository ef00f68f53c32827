// k_assemble.hip -- the multi-GPU frame assembly (rt_assemble_row_bands, rt_assemble_row_bands_rgb8).  Nothing here
// traces: the unit takes the context header for fail, RT_HIP and is_device_ptr, and none of the device headers.
// Row-band layout (distributed.py): frame row y is in band b = y / band_rows, dealt to rank
// b % world, which packed it at slot row (b / world) * band_rows + y % band_rows.  After the
// all-gather (slots in rank order) one launch puts every row at its y -- the GTK thread's
// apply_line (debug_window.rs:147-163) for all ranks at once.  A contiguous tile per rank is the
// case band_rows = slot_rows.
#include "rt_ctx.h"

namespace {

__device__ __forceinline__ const uint8_t* slot_row(const uint8_t* g, size_t gstride, int world, int slot_rows, int band, int y) {   // of frame row y
  const int b = y / band;
  return g + ((size_t)(b % world) * slot_rows + (size_t)(b / world) * band + y % band) * gstride;
}

// One workgroup per row, 16-byte copies when every address allows.
__global__ __launch_bounds__(256) void assemble_bands_kernel(const uint8_t* __restrict__ g, size_t gstride, int world,
                                                             int slot_rows, int band, size_t row_bytes,
                                                             uint8_t* __restrict__ f, size_t fstride, int vec16) {
  const int y = blockIdx.x;
  const uint8_t* s = slot_row(g, gstride, world, slot_rows, band, y);
  uint8_t* d = f + (size_t)y * fstride;
  if (vec16) {
    for (size_t i = threadIdx.x; i < row_bytes / 16; i += blockDim.x) ((uint4*)d)[i] = ((const uint4*)s)[i];
  } else {
    for (size_t i = threadIdx.x; i < row_bytes; i += blockDim.x) d[i] = s[i];
  }
}

// The same placement from packed RGB8 slot rows (3 bytes per pixel, rt_render_row_bands_rgb8) into
// RGBA8 frame rows with A = 255: the all-gather moves 3/4 of the bytes.  One workgroup per row.
// vec: 4 pixels per thread and iteration -- three 4-byte loads (12 bytes = 4 RGB pixels) and one
// 16-byte store -- when the slot rows are 4-byte and the frame rows 16-byte aligned and the width
// is a multiple of 4; otherwise one pixel per thread (3 byte loads, one 4-byte store).
__global__ __launch_bounds__(256) void assemble_bands_rgb_kernel(const uint8_t* __restrict__ g, size_t gstride,
                                                                 int world, int slot_rows, int band, int width,
                                                                 uint8_t* __restrict__ f, size_t fstride, int vec) {
  const int y = blockIdx.x;
  const uint8_t* s = slot_row(g, gstride, world, slot_rows, band, y);
  uint32_t* d = (uint32_t*)(f + (size_t)y * fstride);
  if (vec) {
    const uint32_t* s4 = (const uint32_t*)s;
    for (int q = threadIdx.x; q < width / 4; q += blockDim.x) {
      const uint32_t w0 = s4[3 * q], w1 = s4[3 * q + 1], w2 = s4[3 * q + 2];
      uint4 o;
      o.x = (w0 & 0xFFFFFFu) | 0xFF000000u;
      o.y = (w0 >> 24) | ((w1 & 0xFFFFu) << 8) | 0xFF000000u;
      o.z = (w1 >> 16) | ((w2 & 0xFFu) << 16) | 0xFF000000u;
      o.w = (w2 >> 8) | 0xFF000000u;
      ((uint4*)d)[q] = o;
    }
    return;
  }
  for (int x = threadIdx.x; x < width; x += blockDim.x) {
    const uint8_t* p = s + (size_t)x * 3;
    d[x] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | (255u << 24);
  }
}

}  // namespace

using namespace rt;

// What both entries ask of the slots: every rank's slot holds its bands, and the kernels' int arithmetic holds the slots.
static int slots_ok(uint32_t world, uint32_t slot_rows, uint32_t band_rows, uint32_t height) {
  const uint64_t bands = ((uint64_t)height + band_rows - 1) / band_rows, per_rank = (bands + world - 1) / world;
  if ((uint64_t)slot_rows < per_rank * band_rows)
    return fail(RT_ERR_INVALID, "slot of %u rows holds fewer than %llu bands of %u rows", slot_rows,
                (unsigned long long)per_rank, band_rows);
  if (slot_rows > (1u << 24) || (uint64_t)slot_rows * world > (1u << 30)) return fail(RT_ERR_INVALID, "slot too large");
  return RT_OK;
}

extern "C" {

int rt_assemble_row_bands(const uint8_t* gathered, size_t gathered_stride, uint32_t world, uint32_t slot_rows,
                          uint32_t band_rows, uint32_t height, size_t row_bytes, uint8_t* frame, size_t frame_stride,
                          void* stream) {
  if (!gathered || !frame) return fail(RT_ERR_INVALID, "null argument");
  if (world == 0 || band_rows == 0) return fail(RT_ERR_INVALID, "world and band_rows must be > 0");
  if (height == 0 || row_bytes == 0) return RT_OK;
  if (height > (1u << 24)) return fail(RT_ERR_INVALID, "too many rows");
  RT_TRY(slots_ok(world, slot_rows, band_rows, height));
  if (gathered_stride < row_bytes || frame_stride < row_bytes) return fail(RT_ERR_INVALID, "row stride < row bytes");
  if (!is_device_ptr(gathered) || !is_device_ptr(frame)) return fail(RT_ERR_INVALID, "frame assembly takes device pointers");
  const bool v16 = (((uintptr_t)gathered | (uintptr_t)frame | gathered_stride | frame_stride | row_bytes) & 15) == 0;
  hipLaunchKernelGGL(assemble_bands_kernel, dim3(height), dim3(256), 0, (hipStream_t)stream, gathered, gathered_stride,
                     (int)world, (int)slot_rows, (int)band_rows, row_bytes, frame, frame_stride, v16 ? 1 : 0);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

int rt_assemble_row_bands_rgb8(const uint8_t* gathered, size_t gathered_stride, uint32_t world, uint32_t slot_rows,
                               uint32_t band_rows, uint32_t height, uint32_t width, uint8_t* frame, size_t frame_stride,
                               void* stream) {
  if (!gathered || !frame) return fail(RT_ERR_INVALID, "null argument");
  if (world == 0 || band_rows == 0) return fail(RT_ERR_INVALID, "world and band_rows must be > 0");
  if (height == 0 || width == 0) return RT_OK;
  if (height > (1u << 24) || width > (1u << 24)) return fail(RT_ERR_INVALID, "frame too large");
  RT_TRY(slots_ok(world, slot_rows, band_rows, height));
  if (gathered_stride < (size_t)width * 3 || frame_stride < (size_t)width * 4) return fail(RT_ERR_INVALID, "row stride < row bytes");
  if ((((uintptr_t)frame) | frame_stride) & 3) return fail(RT_ERR_INVALID, "frame rows must be 4-byte aligned");
  if (!is_device_ptr(gathered) || !is_device_ptr(frame)) return fail(RT_ERR_INVALID, "frame assembly takes device pointers");
  const bool vec = (width & 3) == 0 && (((uintptr_t)gathered | gathered_stride) & 3) == 0 &&
                   (((uintptr_t)frame | frame_stride) & 15) == 0;
  hipLaunchKernelGGL(assemble_bands_rgb_kernel, dim3(height), dim3(256), 0, (hipStream_t)stream, gathered, gathered_stride,
                     (int)world, (int)slot_rows, (int)band_rows, (int)width, frame, frame_stride, vec ? 1 : 0);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

}  // extern "C"
