// aa_plan.h -- what the adaptive anti-aliasing pass (k_aa.hip: rt_antialias, rt_antialias_row_bands) needs for its
// edge pixels once the classify kernel has counted them: the sub-pixel grid of a level, the most requests a pass can
// make, and the layout of the pass's one work allocation.  Pure host code, no HIP: tested on the CPU by
// tests/test_aa_plan_host.py the way tests/test_ray_paths_host.py tests paths_plan.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#define RT_AA_MAX_LEVEL 4
#define RT_AA_HAVE_WORDS 5  // have bits per edge pixel, in 64-bit words: (2^4 + 1)^2 = 289 bits
static_assert(((1 << RT_AA_MAX_LEVEL) + 1) * ((1 << RT_AA_MAX_LEVEL) + 1) <= 64 * RT_AA_HAVE_WORDS,
              "one have bit per grid point of the deepest level");

namespace rt {

constexpr size_t RT_AA_COL_BYTES = 32;    // a grid point's colour: four doubles (k_aa.hip AaCol)
constexpr size_t RT_AA_REQ_BYTES = 8;     // a request: (edge pixel, grid point) as uint2
struct AaPlan {
  enum Status { OK, NOTHING, TOO_MANY } status;
  int size;              // grid points per side: (1 << level) + 1
  size_t max_new;        // the largest pass: (2^p + 1)^2 - (2^(p-1) + 1)^2 over p = 1..level (0 at level 0)
  size_t cap;            // requests the list holds: n_edges * max_new, at most 0xffffffff
  size_t col_off, have_off, req_off;   // the colour grids, the have bits, the request list inside the allocation
  size_t bytes;          // the allocation
};

// level: 0..RT_AA_MAX_LEVEL (the caller has clamped and refused); n_edges: the classify kernel's count.
inline AaPlan plan_aa(int level, uint32_t n_edges) {
  AaPlan p = {AaPlan::OK, (1 << level) + 1, 0, 0, 0, 0, 0, 0};
  if (n_edges == 0) { p.status = AaPlan::NOTHING; return p; }
  for (int q = 1; q <= level; ++q) {
    const size_t a = ((size_t)1 << q) + 1, b = ((size_t)1 << (q - 1)) + 1;
    if (a * a - b * b > p.max_new) p.max_new = a * a - b * b;
  }
  p.cap = (size_t)n_edges * p.max_new;
  if (p.cap > 0xffffffffull) { p.status = AaPlan::TOO_MANY; return p; }
  const size_t per_col = (size_t)p.size * p.size * RT_AA_COL_BYTES, per_have = RT_AA_HAVE_WORDS * 8;
  p.have_off = (size_t)n_edges * per_col;
  p.req_off = p.have_off + (size_t)n_edges * per_have;
  p.bytes = p.req_off + p.cap * RT_AA_REQ_BYTES + 256;
  return p;
}

}  // namespace rt
