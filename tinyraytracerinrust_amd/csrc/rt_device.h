// rt_device.h -- the gfx950 (MI355X, CDNA4) device core of the TinyRaytracer render path: the
// reference's per-ray algorithm (get_ray_color and everything it calls) as device functions, shared
// by every kernel translation unit (k_rows.hip, k_wavefront.hip, k_aa.hip, ...) and by the
// scene-specialised programs that hipRTC compiles at scene upload (their text: spec_text.cpp; RT_SPEC).
//
// One thread per pixel; each 64-lane wave owns an 8x8 pixel tile (coherent primary rays,
// fewer divergent CSG/shade branches than a 64x1 row strip).  All arithmetic is IEEE f64 with NO
// contraction (Rust never fuses): every TU is compiled with -ffp-contract=off and the pragma
// below.  sqrt and division lower to correctly rounded sequences on gfx950 (verified bit-exact
// against glibc, profiles/r01_libm_probe.txt); acos is rt_acos (rt_math.h: 1 ulp from glibc on
// ~0.4% of inputs, and far fewer registers than ocml's); sin comes from ocml and may differ from
// glibc by 1 ulp (DESIGN.md "Parity").
//
// The reference's recursion (get_ray_color calling itself for refraction and reflection,
// raytracer.rs:242-280) becomes an explicit per-lane frame stack combined in the same
// post-order: child colour C folds into its parent as in_range(A + in_range(C * w)) where
// A = parent.intensify(1 - w) -- exactly the `final.intensify(1-w) + R.intensify(w)` of
// raytracer.rs:256-257 / :278-279.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/rt_abi.h"
#else                                // hipRTC (the specialised programs): no libc headers
#define INFINITY __builtin_inf()
using __hip_internal::size_t;
#endif

#pragma clang fp contract(off)

// The parts, each including only what stands above it (the Makefile's SPEC_HDRS lists them for the
// build and for the text the specialised programs compile against):
#include "rt_tunables.h"             // numeric tunables and their defaults
#include "rt_core.h"                 // correctly rounded cores, DS, vectors and colours, primitives, hit filters
#include "rt_walks.h"                // conservative culling, the hierarchy walks, nearest hit, shadow rays
#include "rt_trace.h"                // shading inputs, recorders, frame storage, trace, trace_deferred
#include "rt_bodies.h"               // camera rays, tile and band indexing, stores, the kernels' bodies
