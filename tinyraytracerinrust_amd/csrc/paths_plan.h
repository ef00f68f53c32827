// paths_plan.h -- how the batched ray paths (k_paths.hip: rt_ray_paths_offsets, rt_ray_paths) partition their work:
// the exclusive scan of n per-sample ray counts into uint64 offsets, and a sample's segment of the caller's record
// buffer.  Pure host code, no HIP (the segment rule is shared with the fill kernel through RT_PATHS_FN): tested on
// the CPU by tests/test_ray_paths_host.py the way tests/test_launch_plan.py tests launch_plan.h.
//
// The scan is the usual three steps and no workgroup ever waits for another one (no look-back, no tickets):
//   1. sums   one workgroup per block of RT_SCAN_BLOCK counts: the block's sum;
//   2. top    ONE workgroup scans the block sums in place, RT_SCAN_BLOCK of them per round, carrying the running
//             total from round to round, and appends the grand total;
//   3. write  one workgroup per block again: the block's own exclusive scan plus its scanned sum -> offsets.
// n <= RT_SCAN_BLOCK takes step 3 alone (a single workgroup, base 0).  The top workgroup serves at most
// RT_SCAN_TOP_MAX block sums, so n <= RT_SCAN_BLOCK * RT_SCAN_TOP_MAX = 2^26 samples (eight 4K frames' pixel
// centres); more is refused (RT_ERR_UNSUPPORTED) rather than given a third level nobody has asked for.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RT_PATHS_FN __host__ __device__ inline
#else
#define RT_PATHS_FN inline
#endif

namespace rt {

constexpr uint32_t RT_SCAN_THREADS = 256;                        // threads of a scan workgroup
constexpr uint32_t RT_SCAN_ITEMS = 4;                            // consecutive elements per thread
constexpr uint32_t RT_SCAN_BLOCK = RT_SCAN_THREADS * RT_SCAN_ITEMS;   // elements per workgroup: 1024
constexpr uint32_t RT_SCAN_TOP_MAX = 1u << 16;                   // block sums the top workgroup scans (64 rounds)
constexpr uint64_t RT_SCAN_MAX_N = (uint64_t)RT_SCAN_BLOCK * RT_SCAN_TOP_MAX;
// records one call can address: the order table holds absolute 32-bit record indices
constexpr uint64_t RT_PATHS_MAX_RECORDS = 0x7fffffffull;

struct ScanPlan {
  enum Status { OK, NOTHING, TOO_MANY } status;
  uint32_t n_blocks;      // workgroups of steps 1 and 3 (the single-workgroup path: 1)
  uint32_t last_block;    // elements of the last block, 1..RT_SCAN_BLOCK
  bool two_level;         // steps 1 and 2 run (n > RT_SCAN_BLOCK)
  uint32_t top_rounds;    // rounds of the top workgroup, ceil(n_blocks / RT_SCAN_BLOCK); 0 on the single path
  uint64_t sums_bytes;    // the block sums' table: (n_blocks + 1) uint64, 0 on the single path
};

inline ScanPlan plan_scan(uint64_t n) {
  ScanPlan p = {ScanPlan::OK, 0, 0, false, 0, 0};
  if (n == 0) { p.status = ScanPlan::NOTHING; return p; }
  if (n > RT_SCAN_MAX_N) { p.status = ScanPlan::TOO_MANY; return p; }
  p.n_blocks = (uint32_t)((n + RT_SCAN_BLOCK - 1) / RT_SCAN_BLOCK);
  p.last_block = (uint32_t)(n - (uint64_t)(p.n_blocks - 1) * RT_SCAN_BLOCK);
  p.two_level = p.n_blocks > 1;
  if (p.two_level) {
    p.top_rounds = (p.n_blocks + RT_SCAN_BLOCK - 1) / RT_SCAN_BLOCK;
    p.sums_bytes = ((uint64_t)p.n_blocks + 1) * 8;
  }
  return p;
}

// Sample i's segment of a record buffer of `cap` records, from its two offsets: [o0, min(o1, cap)), and the empty
// segment (at 0) when o0 > o1 or o0 > cap.  Whatever the offsets hold, begin + len <= cap.
struct PathSegment { uint64_t begin; uint32_t len; };
RT_PATHS_FN PathSegment path_segment(uint64_t o0, uint64_t o1, uint64_t cap) {
  PathSegment s = {0, 0};
  if (o0 > o1 || o0 > cap) return s;
  const uint64_t end = o1 < cap ? o1 : cap;
  const uint64_t len = end - o0;
  s.begin = o0;
  s.len = len > RT_PATHS_MAX_RECORDS ? (uint32_t)RT_PATHS_MAX_RECORDS : (uint32_t)len;
  return s;
}

}  // namespace rt
