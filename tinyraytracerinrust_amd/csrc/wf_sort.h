// wf_sort.h -- the in-tree bucket sort of the wavefront path (wf_sort.hip): its bin limits, which size the
// callers' scratch (wf_plan.h, on a CPU too), and its prototype for the HIP units that call it.
#pragma once
#include <stdint.h>

#define RT_BS_MAX_BINS 4096     // bins of one sort at most: one LDS histogram
#define RT_BS_FUSED_BINS 2048   // sorts of at most this many bins skip the scan launch (wf_sort.hip)

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// Sorts n (key, value) pairs by bin = min(key >> shift, nb - 1); the arguments: wf_sort.hip
extern "C" hipError_t rt_wf_bucket_sort(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                                        uint32_t* vals_out, uint32_t n, const uint32_t* n_dev, uint32_t nb, int shift,
                                        uint32_t* cnt, bool zero_cnt, hipStream_t stream, bool counted = false);
#endif
