// rt_tunables.h -- the numeric tunables of the device core (rt_device.h includes this first), each with
// the default the product is built with.  `make diag DIAG=-DNAME=value` builds an A/B library with
// another value, and the specialised programs of such a library take it through their prelude
// (spec_text.cpp).  One line per tunable: what it sizes, and where DESIGN.md holds its sweep.
// (RT_TILE_W, the tile's width, is rt_blob.h's: the host's tile arithmetic shares it.)
#pragma once

// Waves per SIMD of the row kernels (amdgpu_waves_per_eu: the VGPR budget is 512 / N), by kernel mode.
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 4             // ray-tree refraction kernels, 128 VGPRs (section 2 "The kernel": occupancy and scratch)
#endif
#ifndef RT_WAVES_PER_EU_NOREFR
#define RT_WAVES_PER_EU_NOREFR 5      // reflection-only megakernel, at most 102 VGPRs (section 2 "The kernel"; section 7, the re-sweep)
#endif
#ifndef RT_WAVES_PER_EU_CHAIN
#define RT_WAVES_PER_EU_CHAIN 4       // refraction-chain kernel: no spill, the traffic budget over 5 % (section 2 "Kernel modes")
#endif
#ifndef RT_WAVES_PER_EU_DEFERRED
#define RT_WAVES_PER_EU_DEFERRED 7    // deferred-shadow kernel (section 7: 5 / 6 / 8 waves are slower)
#endif

// Frame storage in LDS per one-wave workgroup (rt_trace.h "Frame-stack slots", "The wave's frame POOL").
#ifndef RT_LDS_FRAMES
#define RT_LDS_FRAMES 2               // per-lane colour frames, reflection-only and ray-tree modes: 4 KB (section 2 "The kernel")
#endif
#ifndef RT_LDS_FRAMES_CHAIN
#define RT_LDS_FRAMES_CHAIN 0         // per-lane colour frames, chain mode: none, every frame in the pool (section 2 "Round 6")
#endif
#ifndef RT_LDS_RFRAMES
#define RT_LDS_RFRAMES 1              // per-lane pending-reflection frames, ray-tree mode: 3.5 KB (section 7)
#endif
#ifndef RT_LDS_POOL_REFL
#define RT_LDS_POOL_REFL 0            // wave-pool slots, reflection-only mode: no pool, its chains are short (section 2 "Kernel modes")
#endif
#ifndef RT_LDS_POOL_CHAIN
#define RT_LDS_POOL_CHAIN 320         // wave-pool slots, chain mode: 8 KB, 5 waves/SIMD (section 2 "Round 6"; section 7)
#endif

// Deferred-shadow kernel (rt_trace.h trace_deferred, rt_bodies.h deferred_body).
#ifndef RT_SH_TRCAP
#define RT_SH_TRCAP 128               // shadow results per round in the wave's LDS window: hits per round = min(64, TRCAP / lights)
#endif
#ifndef RT_SPLIT_MAX_LOG2
#define RT_SPLIT_MAX_LOG2 3           // a costly tile goes to at most 2^3 = 8 waves (section 7: 16 changes nothing)
#endif
