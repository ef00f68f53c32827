// k_wf_pairs.hip -- the wavefront path's pair path: a level's traversals as (ray, object) work items sorted by
// object (DESIGN.md §2 "Wavefront path").  Its kernels, its arrays (wfp_arena) and one level's launches (wfp_level)
// for k_wavefront.hip's launch_wavefront; the sizes, layouts and choices are wf_plan.h's.
#include <algorithm>

#include "rt_wavefront.h"
#include "rt_ctx.h"
#include "wf_sort.h"

using namespace rt;

namespace {
// ---------------------------------------------------------------- wavefront pair path
// A level's rays are incoherent after a few bounces through scenes of many objects (fractal.scene:
// 171 objects, glass spheres in hollow CSG cubes).  A wave that walks the hierarchy for 64 scattered
// rays visits the union of their paths: on fractal.scene only 14 % / 22 % of the lanes are active in
// a secondary / shadow leaf evaluation, and every level's pass takes as long as a wave's walk over
// most of the scene (0.6-2 ms even for 25 000 rays).  The pair path splits the traversal into
// (ray, object) work items and evaluates them object by object:
//   wfp_cand_kernel<false>   per ray: the hierarchy walk with box tests only (no leaf), emitting a
//                            pair (object, ray) for every object box the ray meets (through a per-wave
//                            LDS buffer, one atomic per RT_WFP_BUF pairs);
//   sort                     the pairs by object (the in-tree bucket sort, wf_sort.hip), so a wave evaluates ONE
//                            object (scalar loads of its leaves, every lane busy) for 64 different rays;
//   wfp_near_eval_kernel     per pair: the object's nearest accepted distance (leaf tests, CSG filters:
//                            nearest_hit's object body); atomicMin of its bits into the ray's best;
//   wfp_near_tie_kernel      per pair at the ray's best distance: atomicMin of the object index.  The
//                            nearest hit is the least (distance, object) -- exactly nearest_hit's
//                            draw-order first-wins rule (raytracer.rs:141-150);
//   wfp_cand_kernel<true>    per ray with a hit and per light: the shadow ray's candidate objects;
//   sort, wfp_shadow_eval    per pair: the object's filtered hits with EPS < t < dist; a hit of a
//                            zero-transparency object marks the shadow ray opaque, other hits add to
//                            its count.  RtDevScene::shadow_pow (scene.cpp) guarantees the product in
//                            draw order is then 0 or T^count, order-free (raytracer.rs:181-197);
//   wfp_shade_kernel         per ray: wf_ray_core's shading, refraction and reflection decisions with
//                            the folded results, then wf_append, as wf_trace_kernel.
// Every value is computed by the same operations as the traversals; culling stays conservative
// (the candidate walk tests boxes against the whole ray, tmax = infinity for the nearest hit).
#ifndef RT_WFP_BUF
#define RT_WFP_BUF 512          // pairs buffered in LDS per wave before one atomic allocates their slots
#endif
constexpr unsigned long long RT_WFP_NONE = 0x7FF0000000000000ull;   // +inf

// The object's nearest accepted distance for one ray: nearest_hit's body for one object, its best
// starting at +inf (the leaf boxes' tmax only shrinks, as share_prev requires).
__device__ __forceinline__ double wfp_object_nearest(const DS& S, int o, V3 ro, V3 rd, const CullR& cr) {
  const bool cf_ok = const_filter_range(ro, rd);
  cptr<RtObject> O = &S.objects[o];
  const bool fin = wave_finite(ro, rd);
  double best = INFINITY;
  SphereShare shr = {0.0, 0.0, 0.0};
  const int lb = O->leaf_begin, le = lb + O->leaf_count;
  for (int l = lb; l < le; ++l) {
    cptr<RtLeaf> L = &S.leaves[l];
    if (O->leaf_cull) {
      if (L->cull == RT_CULL_ALWAYS) continue;
      if (L->cull == RT_CULL_BOX && !RT_BOX_MAY_HIT(L, blo, bhi, cr, RT_CULL_TMAX(best))) continue;
    }
    double t0 = 0.0, t1 = 0.0;
    const int n = leaf_candidates<true>(L, ro, rd, fin, &t0, &t1, &shr);
    const bool filtered = L->prog_end != L->prog_begin && !(cf_ok && L->filter_const);
    if (n >= 1 && t0 > EPS && t0 < best && (!filtered || leaf_filter(S, L, add(ro, scale(rd, t0))))) best = t0;
    if (n >= 2 && t1 > EPS && t1 < best && (!filtered || leaf_filter(S, L, add(ro, scale(rd, t1))))) best = t1;
  }
  return best;
}

// Filtered hits of the object with EPS < t < dist on one shadow ray (shadow_transparency's body for
// one object); a zero-transparency object stops at its first.
__device__ __forceinline__ uint32_t wfp_object_shadow(const DS& S, int o, V3 p, V3 dir, double dist, const CullR& cr) {
  cptr<RtObject> O = &S.objects[o];
  const bool fin = wave_finite(p, dir);
  const bool cf_ok = const_filter_range(p, dir);
  const CullT tmax = RT_CULL_TMAX(dist);
  const bool zero = O->transparency == 0.0;
  uint32_t cnt = 0;
  SphereShare shr = {0.0, 0.0, 0.0};
  const int lb = O->leaf_begin, le = lb + O->leaf_count;
  for (int l = lb; l < le; ++l) {
    cptr<RtLeaf> L = &S.leaves[l];
    if (O->leaf_cull) {
      if (L->cull == RT_CULL_ALWAYS) continue;
      if (L->cull == RT_CULL_BOX && !RT_BOX_MAY_HIT(L, blo, bhi, cr, tmax)) continue;
    }
    double t0 = 0.0, t1 = 0.0;
    const int n = leaf_candidates<true>(L, p, dir, fin, &t0, &t1, &shr);
    const bool filtered = L->prog_end != L->prog_begin && !(cf_ok && L->filter_const);
    if (n >= 1 && t0 > EPS && t0 < dist && (!filtered || leaf_filter(S, L, add(p, scale(dir, t0))))) {
      ++cnt;
      if (zero) return cnt;
    }
    if (n >= 2 && t1 > EPS && t1 < dist && (!filtered || leaf_filter(S, L, add(p, scale(dir, t1))))) {
      ++cnt;
      if (zero) return cnt;
    }
  }
  return cnt;
}

// Ray of slot j of level d (level 0: the pixel slot's camera ray).
__device__ __forceinline__ bool wf_get_ray(const RtDevScene& S, const WfLevel& lv, int d, uint32_t j, WfRows rows, V3* ro,
                                           V3* rd) {
  if (d == 0) {
    int x, r, y;
    if (!wf_pixel(S, j, rows, &x, &r, &y)) return false;
    camera_ray_px(S, x, y, ro, rd);
    return true;
  }
  *ro = {lv.ox[j], lv.oy[j], lv.oz[j]};
  *rd = {lv.dx[j], lv.dy[j], lv.dz[j]};
  return true;
}

// One wave per 64 rays of level d (in key order).  SHADOW = false: every object whose box the ray
// meets; true: per light, every object whose box the shadow segment meets (objects of transparency 1
// skipped, as shadow_transparency does).
// Each lane walks its own path through the hierarchy (one 32-byte RtTravC record per step, which
// carries the object's box and flags): a wave-uniform walk visits the union of its 64 rays' paths,
// measured 4-20 % slower here (profiles/r03m_pairs_fractal_timing.txt).
// A step's record load is the walk's latency: one dependent per-lane load per node, ~100 of them
// per deep ray on fractal.scene -- the deep levels' dispatches last 45-90 us with a few hundred
// waves because each wave is that chain (SQ_WAVE_CYCLES counts quad-cycles: the round-3 "8-15 k
// cycles" per wave are 32-60 k, 15-30 us).  LDS_TRAV: the workgroup (WG_WAVES waves) first copies
// the hierarchy into LDS and the walks read it there.  Loading the next record beside the box test
// (the pre-order successor, the next step unless a group misses) measured 9 % slower on the fractal
// frame (6.02 -> 6.58 ms, profiles/r07q_fractal.txt): kept out.
#ifndef RT_WFP_CAND_WAVES_N
#define RT_WFP_CAND_WAVES_N 4
#endif
constexpr int RT_WFP_CAND_WAVES = RT_WFP_CAND_WAVES_N;
#ifndef RT_WFP_MAX_RANGES_LOG2
#define RT_WFP_MAX_RANGES_LOG2 2                     // at most 4 hierarchy ranges per ray (below)
#endif
#ifndef RT_WFP_HITSORT_MAX_D
#define RT_WFP_HITSORT_MAX_D 1000                    // levels from this depth on skip the hit-point sort
#endif
#ifndef RT_WFP_RANGE_PASSES
#define RT_WFP_RANGE_PASSES 8                        // ... while the items fill the grid at most 8 times (4: +0.8 %)
#endif
#ifndef RT_WFP_NEAR_RANGES_LOG2
#define RT_WFP_NEAR_RANGES_LOG2 1                    // the nearest pass's walks: at most 2 ranges (8 measured slower)
#endif
// n_dev != nullptr (device-driven levels): the level's ray count is min(*n_dev, A.cap), read here; the
// grid is then a fixed number of workgroups that take the level's rays grid-stride, 64 x WG_WAVES at a
// time (the hierarchy staged in LDS once per workgroup).
template <bool SHADOW, bool LDS_TRAV>
__global__ __launch_bounds__(64 * RT_WFP_CAND_WAVES) void wfp_cand_kernel(RtDevScene S, WfArena A, WfPairs P, int d,
                                                                          uint32_t n, const uint32_t* n_dev, WfRows rows,
                                                                          uint32_t* __restrict__ hcnt) {
  constexpr int WW = LDS_TRAV ? RT_WFP_CAND_WAVES : 1;
  __shared__ uint32_t sk_all[WW][RT_WFP_BUF], sv_all[WW][RT_WFP_BUF];
  extern __shared__ __attribute__((aligned(16))) uint8_t s_trav[];
  // hcnt != nullptr: the pairs' histogram by object for the bucket sort (its histogram launch skipped),
  // counted in LDS (after the staged hierarchy) and added to hcnt once per workgroup
  uint32_t* const s_hist = (uint32_t*)(s_trav + (LDS_TRAV ? (size_t)S.n_trav * sizeof(RtTravC) : 0));
  const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
  uint32_t* sk = sk_all[LDS_TRAV ? wv : 0];
  uint32_t* sv = sv_all[LDS_TRAV ? wv : 0];
  if (n_dev) n = min(*n_dev, A.cap);
  // Hierarchy ranges: a small level's rays are too few to fill the grid, and its time is the longest
  // walk of one lane (~100-600 dependent node steps).  There the node array is cut into K equal
  // contiguous ranges and a lane walks one (ray, range) item: the walk from a range's first node
  // to its end with the same steps (skip pointers only jump forward; a group that misses covers only
  // nodes the ray misses too, as its box holds its objects' boxes).  Ancestors outside the range go
  // untested, so an item may emit pairs the whole walk culls: a superset, which the evaluations
  // resolve exactly.  K: a power of two, at most 2^RT_WFP_MAX_RANGES_LOG2, n x K within RT_WFP_RANGE_PASSES grids.
  const uint32_t nthreads = gridDim.x * (64u * WW);
  uint32_t lk = 0;
  while (lk < (SHADOW ? RT_WFP_MAX_RANGES_LOG2 : RT_WFP_NEAR_RANGES_LOG2) &&
         ((uint64_t)n << (lk + 1)) <= (uint64_t)nthreads * RT_WFP_RANGE_PASSES)
    ++lk;
  const uint32_t items = n << lk;
  if (blockIdx.x * (64u * WW) >= items) return;              // no ray for this workgroup: no staging either
  if (hcnt)
    for (uint32_t b = threadIdx.x; b < (uint32_t)S.n_objects; b += blockDim.x) s_hist[b] = 0;
  if constexpr (LDS_TRAV) {                                   // the hierarchy into LDS, once per workgroup
    const uint4* g = (const uint4*)S.trav_c;
    uint4* l = (uint4*)s_trav;
    for (uint32_t q = threadIdx.x; q < (uint32_t)S.n_trav * (sizeof(RtTravC) / 16); q += blockDim.x) l[q] = g[q];
  }
  if (LDS_TRAV || hcnt) __syncthreads();
  const WfLevel lv = wf_level(A, d);
  const DS D = make_ds(S);
  uint32_t nb = 0;                                           // wave-uniform fill of the LDS buffer
  auto wave_sync = []() {                                    // the wave's own buffer: a wave-level barrier
    if constexpr (LDS_TRAV) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  };
  auto flush = [&]() {
    wave_sync();
    uint32_t base = 0;
    if (lane == 0) {
      base = atomicAdd(P.count + (SHADOW ? WFP_SHADOW : WFP_NEAREST), nb);
      // a 32-bit count past 2^31 (the arena's limit) is about to wrap: flag the level as failed (the
      // writes below stay inside the arena; the host reports the overflow instead of using the pairs)
      if (base >= 0x80000000u) atomicOr(P.count + WFP_WRAPPED, 1u);
    }
    base = (uint32_t)__shfl((int)base, 0);
    // the histogram counts the pairs the list holds (a level that overflows it is rendered again, but
    // its sort must still see counts that match the stored keys: no unwritten slot is read)
    for (uint32_t q = (uint32_t)lane; q < nb; q += 64)
      if (base + q < P.cap) {
        P.key[base + q] = sk[q];
        P.val[base + q] = sv[q];
        if (hcnt) atomicAdd(&s_hist[sk[q]], 1u);
      }
    wave_sync();
    nb = 0;
  };
  auto emit = [&](bool h, uint32_t ob, uint32_t id) {
    const uint64_t m = __ballot(h);
    if (!m) return;
    const uint32_t c = (uint32_t)__popcll(m);
    if (nb + c > RT_WFP_BUF) flush();
    if (h) {
      const uint32_t q = nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      sk[q] = ob;
      sv[q] = id;
    }
    nb += c;
  };
  auto walk = [&](bool act0, V3 o, V3 dir, double tmax, uint32_t id, int t0, int nt) {   // nodes [t0, nt)
    const CullRayF cr = cull_ray_f(o, dir);
    const float tm = (float)tmax;
    const RtTravC* __restrict__ TR = LDS_TRAV ? (const RtTravC*)(const void*)s_trav : S.trav_c;
    int t = act0 ? t0 : nt;
    while (__ballot(t < nt)) {
      bool h = false;
      int ob = 0;
      if (t < nt) {
        const RtTravC T = TR[t];
        const bool in = fbox_may_hit(T.lo, T.hi, cr, tm);
        const int cull = (int)((T.skip_flags >> 28) & 3u);
        if (T.obj < 0) {
          t = in ? t + 1 : (int)(T.skip_flags & 0x0fffffffu);
        } else {
          ++t;
          ob = T.obj;
          h = cull != RT_CULL_ALWAYS && !(SHADOW && (T.skip_flags >> 30)) && (cull != RT_CULL_BOX || in);
        }
      }
      emit(h, (uint32_t)ob, id);
    }
  };
  for (uint32_t base = blockIdx.x * (64u * WW); base < items; base += nthreads) {   // wave-uniform
    const uint32_t q = base + threadIdx.x, i = q >> lk, rg = q & ((1u << lk) - 1u);
    // this item's range of the node array (the whole array when K = 1)
    const int t0 = (int)(((uint32_t)S.n_trav * rg) >> lk), t1 = (int)(((uint32_t)S.n_trav * (rg + 1u)) >> lk);
    bool live = q < items;
    uint32_t j = i;
    V3 ro = {0.0, 0.0, 0.0}, rd = {0.0, 0.0, 0.0};
    if (live) {
      j = SHADOW ? P.hperm[i] : (d > 0 && A.perm) ? A.perm[i] : i;
      if (!SHADOW) live = wf_get_ray(S, lv, d, j, rows, &ro, &rd);
    }
    if constexpr (!SHADOW) {
      if (q < items && rg == 0) { P.tmin[j] = RT_WFP_NONE; P.omin[j] = 0x7fffffff; }   // slots outside the frame too
      // A bound on the nearest hit: the object whose hit spawned the ray, evaluated first (a ray that
      // refracted into or reflects inside a closed shape meets it again).  The walk then tests boxes
      // against [0, cull_tmax(bound)] only -- conservative, as nearest_hit's running best is; the
      // parent's own pair is still emitted by the walk (its box contains the bound's point).
      double bound = INFINITY;
      if (d > 0) {
        const int32_t par = live ? lv.par[j] : -1;
        const CullR cr = RT_CULL_RAY(ro, rd);
        // the children of one shading wave: mostly one parent
        wf_for_each_uniform(__ballot(live && par >= 0), live, par, lane,
                            [&](int pu) { bound = wfp_object_nearest(D, pu, ro, rd, cr); });
      }
      walk(live, ro, rd, bound < INFINITY ? cull_tmax(bound) : INFINITY, j, t0, t1);
    } else {
      const int32_t oi = live ? P.omin[j] : 0x7fffffff;
      const bool hit = live && oi != 0x7fffffff;
      V3 p = {0.0, 0.0, 0.0};
      if (hit) p = {P.px[j], P.py[j], P.pz[j]};                     // wfp_hit_key_kernel
      for (int k = 0; k < D.n_lights; ++k) {
        V3 sdir = {0.0, 0.0, 0.0};
        double tmax = 0.0;
        const uint32_t s = j * (uint32_t)D.n_lights + (uint32_t)k;
        if (hit) {
          cptr<RtLight> lt = &D.lights[k];
          const V3 l = sub(ld3(lt->p), p);
          double ll, ill;
          len_inv(l, &ll, &ill);
          sdir = scale(l, ill);
          tmax = cull_tmax(ll);
          if (rg == 0) {
            P.kcnt[s] = 0;
            P.opq[s] = 0;
          }
        }
        walk(hit, p, sdir, tmax, s, t0, t1);
      }
    }
  }
  flush();
  if (hcnt) {                                                // every wave of the workgroup is done
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (uint32_t)S.n_objects; b += blockDim.x)
      if (s_hist[b]) atomicAdd(&hcnt[b], s_hist[b]);
  }
}

// One lane per sorted pair: the waves see one object (two at a run boundary): scalarised over the
// distinct objects of the wave as shade_inputs does, so every scene read is a scalar load.
__global__ __launch_bounds__(64) void wfp_near_eval_kernel(RtDevScene S, WfArena A, WfPairs P, int d, WfRows rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t np = min(P.count[WFP_NEAREST], P.cap);     // pairs of this level's nearest pass (device)
  const WfLevel lv = wf_level(A, d);
  const DS D = make_ds(S);
  for (uint32_t base = blockIdx.x * 64u; base < np; base += gridDim.x * 64u) {   // wave-uniform bounds
    const uint32_t i = base + (uint32_t)lane;
    bool live = i < np;
    uint32_t o = 0xffffffffu, j = 0;
    V3 ro = {0.0, 0.0, 0.0}, rd = {0.0, 0.0, 0.0};
    if (live) {
      o = P.key_s[i];
      j = P.val_s[i];
      live = wf_get_ray(S, lv, d, j, rows, &ro, &rd);
    }
    const CullR cr = RT_CULL_RAY(ro, rd);
    double best = INFINITY;
    wf_for_each_uniform(__ballot(live), live, o, lane,
                        [&](uint32_t ou) { best = wfp_object_nearest(D, (int)ou, ro, rd, cr); });
    if (live) {
      P.tp[i] = best;
      if (best < INFINITY) atomicMin(&P.tmin[j], (unsigned long long)__double_as_longlong(best));
    }
  }
}

__global__ __launch_bounds__(256) void wfp_near_tie_kernel(WfPairs P) {
  const uint32_t np = min(P.count[WFP_NEAREST], P.cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
    const double t = P.tp[i];
    if (!(t < INFINITY)) continue;
    const uint32_t j = P.val_s[i];
    if ((unsigned long long)__double_as_longlong(t) == P.tmin[j]) atomicMin(&P.omin[j], (int32_t)P.key_s[i]);
  }
}

// Per ray of the level, after the nearest-hit folds: the hit point (wf_ray_core's p) and a coherence
// key for the shadow and shading passes: the hit object above the top `cbits` bits of the Morton code
// of the hit point's cell (a wave then shades one object -- shade_inputs' waterfall runs once -- and
// its shadow rays start close together); misses sort last.
__global__ __launch_bounds__(256) void wfp_hit_key_kernel(RtDevScene S, WfArena A, WfPairs P, int d, uint32_t n,
                                                          const uint32_t* n_dev, WfRows rows, int cbits) {
  if (n_dev) n = min(*n_dev, A.cap);
  const WfLevel lv = wf_level(A, d);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t j = (d > 0 && A.perm) ? A.perm[i] : i;
    V3 ro, rd;
    uint32_t key = (uint32_t)S.n_objects << cbits;
    if (wf_get_ray(S, lv, d, j, rows, &ro, &rd) && P.omin[j] != 0x7fffffff) {
      const V3 p = add(ro, scale(rd, __longlong_as_double((long long)P.tmin[j])));
      P.px[j] = p.x; P.py[j] = p.y; P.pz[j] = p.z;
      const uint32_t cell = (wf_key(A, p, V3{0.0, 0.0, 0.0}) & 0x07ffffffu) >> (27 - cbits);
      key = ((uint32_t)P.omin[j] << cbits) | (cbits ? cell : 0u);
    }
    P.hkey[i] = key;
    P.hval[i] = j;
  }
}

__global__ __launch_bounds__(64) void wfp_shadow_eval_kernel(RtDevScene S, WfPairs P) {
  const int lane = threadIdx.x & 63;
  const uint32_t np = min(P.count[WFP_SHADOW], P.cap);      // pairs of this level's shadow pass (device)
  const DS D = make_ds(S);
  for (uint32_t base = blockIdx.x * 64u; base < np; base += gridDim.x * 64u) {   // wave-uniform bounds
    const uint32_t i = base + (uint32_t)lane;
    const bool live = i < np;
    uint32_t o = 0xffffffffu, s = 0;
    V3 p = {0.0, 0.0, 0.0}, sdir = {0.0, 0.0, 0.0};
    double ll = 0.0;
    if (live) {
      o = P.key_s[i];
      s = P.val_s[i];
      const uint32_t j = s / (uint32_t)S.n_lights, k = s % (uint32_t)S.n_lights;
      p = {P.px[j], P.py[j], P.pz[j]};
      const RtLight& lt = S.lights[k];
      const V3 l = sub(V3{lt.p[0], lt.p[1], lt.p[2]}, p);              // wf_ray_core's light loop
      double ill;
      len_inv(l, &ll, &ill);
      sdir = scale(l, ill);
    }
    const CullR cr = RT_CULL_RAY(p, sdir);
    uint32_t cnt = 0;
    wf_for_each_uniform(__ballot(live), live, o, lane,
                        [&](uint32_t ou) { cnt = wfp_object_shadow(D, (int)ou, p, sdir, ll, cr); });
    if (live && cnt) {
      if (D.objects[o].transparency == 0.0) atomicOr(&P.opq[s], 1u);
      else atomicAdd(&P.kcnt[s], cnt);
    }
  }
}

template <bool REFR, bool FC>
__device__ __forceinline__ void wfp_shade_one(RtDevScene S, WfArena A, WfPairs P, const WfLevel& lv, int d, uint32_t i,
                                              uint32_t n, int lane, WfRows rows, int max_depth) {
  bool live = i < n;
  V3 ro = {0.0, 0.0, 0.0}, rd = {0.0, 0.0, 0.0};
  uint32_t j = i;
  int32_t pix = (int32_t)i;
  if (live) {
    j = P.hperm[i];                                          // hit-point order (wfp_hit_key_kernel)
    live = wf_get_ray(S, lv, d, j, rows, &ro, &rd);
    pix = d > 0 ? lv.pix[j] : (int32_t)j;
  }
  Col L = {0.0, 0.0, 0.0};
  double wt = 0.0, wr = 0.0;
  bool ch_t = false, ch_r = false;
  V3 p = {0.0, 0.0, 0.0}, dt = {0.0, 0.0, 0.0}, dr = {0.0, 0.0, 0.0};
  const uint32_t nl = (uint32_t)S.n_lights;
  const double T = S.shadow_t;
  if (live)
    wf_ray_core<REFR, FC>(
        make_ds(S), ro, rd, d, max_depth,
        [&](double* t) {
          const int32_t oi = P.omin[j];
          if (oi == 0x7fffffff) { *t = INFINITY; return -1; }
          *t = __longlong_as_double((long long)P.tmin[j]);
          return (int)oi;
        },
        [&](int k, V3, V3, double) {
          const uint32_t s = j * nl + (uint32_t)k;
          if (P.opq[s]) return 0.0;
          double tr = 1.0;                                     // shadow_transparency's product, order-free
          for (uint32_t c = P.kcnt[s]; c > 0; --c) {
            tr *= T;
            if (tr == 0.0) return 0.0;
          }
          return tr;
        },
        &L, &wt, &wr, &ch_t, &ch_r, &p, &dt, &dr);
  wf_append(A, lv, d, lane, live, j, pix, L, wt, wr, ch_t, ch_r, p, dt, dr, live ? P.omin[j] : -1);
}

// n_dev != nullptr (device-driven levels): the ray count is min(*n_dev, A.cap); the waves take the
// level's rays grid-stride, 64 at a time (wf_append: one ballot + one atomic per wave and chunk).
// The level's last kernel also closes it (every reader of the pair counts and the sort scratch has
// run): thread 0 checks the pair counts against the lists (a level that emitted more pairs than they
// hold computed wrong nearest hits: the sticky words WFP_NEED / WFP_WRAP, which the host reads once per
// launch), logs and zeroes them, and the grid zeroes the three sorts' scratch -- for the next level, with no
// launches of their own (5 us each on the small levels).
template <bool REFR, bool FC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU_WF))) void wfp_shade_kernel(
    RtDevScene S, WfArena A, WfPairs P, int d, uint32_t n, const uint32_t* n_dev, WfRows rows, int max_depth) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && lane == 0) {
    uint32_t* pc = P.count;
    const uint32_t m = max(pc[WFP_NEAREST], pc[WFP_SHADOW]);
    if (m > P.cap) atomicMax(pc + WFP_NEED, m);
    if (pc[WFP_WRAPPED]) atomicOr(pc + WFP_WRAP, 1u);
    if (d <= RT_WFP_LOG_LEVELS) { pc[wfp_log(d, false)] = pc[WFP_NEAREST]; pc[wfp_log(d, true)] = pc[WFP_SHADOW]; }
    pc[WFP_NEAREST] = pc[WFP_SHADOW] = pc[WFP_WRAPPED] = 0;
  }
  for (uint32_t k = blockIdx.x * 64u + (uint32_t)lane; k < 3u * RT_WFP_BIN_WORDS; k += gridDim.x * 64u) P.bins[k] = 0;
  if (n_dev) n = min(*n_dev, A.cap);
  const WfLevel lv = wf_level(A, d);
  for (uint32_t base = blockIdx.x * 64u; base < n; base += gridDim.x * 64u)   // wave-uniform
    wfp_shade_one<REFR, FC>(S, A, P, lv, d, base + (uint32_t)lane, n, lane, rows, max_depth);
}

}  // namespace

int rt::wfp_lists(rt_ctx* c, const WfPlan& plan, size_t need) {
  const WfListSize s = wf_list_size(c->wfp ? c->wfp_cap : 0, plan.cap, need);
  if (!s.grow) return RT_OK;
  if (s.refused) return fail(RT_ERR_UNSUPPORTED, "%s", s.error);
  c->wfp_cap = 0;
  RT_TRY(grow_device(c->wfp, c->wfp_bytes, wf_list_layout(s.cap).bytes));
  c->wfp_cap = (uint32_t)s.cap;
  return RT_OK;
}

// The pair path's arrays for a level of the plan's launch: per ray (grow-only) and the pair lists as they are.
static int wfp_arena(rt_ctx* c, const WfPlan& plan, const WfArena& A, WfPairs* P) {
  RT_TRY(grow_device(c->wfr, c->wfr_bytes, plan.ray.bytes));
  RT_TRY(wfp_lists(c, plan, 0));
  const WfRayLayout& o = plan.ray;
  const size_t R = plan.rays, cap = c->wfp_cap;
  uint8_t* r = (uint8_t*)c->wfr;
  P->tmin = (unsigned long long*)(r + o.tmin);
  P->omin = (int32_t*)(r + o.omin);
  P->px = (double*)(r + o.px); P->py = P->px + R; P->pz = P->py + R;
  P->kcnt = (uint32_t*)(r + o.kcnt);
  P->opq = (uint32_t*)(r + o.opq);
  P->hkey = (uint32_t*)(r + o.hkey); P->hval = P->hkey + R; P->hkey_s = P->hval + R; P->hperm = P->hkey_s + R;
  const WfListLayout l = wf_list_layout(cap);
  uint8_t* b = (uint8_t*)c->wfp;
  P->cap = (uint32_t)cap;
  P->count = A.count + WFC_PAIRS;
  P->bins = (uint32_t*)(b + l.bins);    // nearest / hit-point / shadow sorts
  P->key = (uint32_t*)(b + l.key); P->val = P->key + cap; P->key_s = P->val + cap; P->val_s = P->key_s + cap;
  P->tp = (double*)(b + l.tp);
  return RT_OK;
}

// One level of the wavefront path through the pair path: candidate pairs, sort by object, pair evaluation and the
// folds, for the nearest hits and then the shadow rays, then the shading pass.  Device-driven: no host
// synchronisation.  The level's ray count is n_ub (known on the host: level 0, n_dev null) or min(*n_dev, cap), read
// by the kernels themselves; the pair counts stay on the device too (the sorts and the evaluations read them).  Grids
// are fixed and the kernels take their work grid-stride, so the host launches every level back to back.  A level whose
// pairs outgrew the lists leaves the sticky word WFP_NEED (checked by the level's shading kernel); the host reads it
// once, after the whole launch, and renders the launch again with lists of that size (launch_wavefront).
int rt::wfp_level(rt_ctx* c, hipStream_t st, const WfPlan& plan, const WfArena& A, int d, uint32_t n_ub,
                  const uint32_t* n_dev, WfRows rows, bool first) {
  WfPairs P;
  RT_TRY(wfp_arena(c, plan, A, &P));
  const uint32_t ncu = (uint32_t)c->n_cu;
  auto grid = [&](uint32_t per_wg, uint32_t max_wg) { return dim3(std::max(1u, std::min((n_ub + per_wg - 1) / per_wg, max_wg))); };
  const dim3 b64(64);
  const uint32_t nobj = (uint32_t)c->dev.n_objects;
  uint32_t* bins[3] = {P.bins, P.bins + RT_WFP_BIN_WORDS, P.bins + 2 * RT_WFP_BIN_WORDS};
  auto launch_cand = [&](bool shadow) {
    uint32_t* hc = plan.counted ? bins[shadow ? 2 : 0] : nullptr;
    with_bool(shadow, [&](auto SH) { with_bool(plan.lds_trav, [&](auto LT) {
      constexpr bool SHADOW = decltype(SH)::value, LDS_TRAV = decltype(LT)::value;
      const size_t lds = plan.trav_lds + plan.hist_lds;
      dim3 g = grid(64, ncu * 64), b = b64;
      if constexpr (LDS_TRAV) {
        // as many workgroups as the CUs hold at once (the LDS-staged hierarchy sets it); they take the level's rays
        // grid-stride and stage the hierarchy once each (16 per CU: on the small levels most only staged and found no ray)
        int& occ = c->wfp_occ[shadow ? 1 : 0];                    // queried once per context and LDS size
        if (occ < 1 || c->wfp_occ_lds[shadow ? 1 : 0] != lds) {
          if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)wfp_cand_kernel<SHADOW, LDS_TRAV>,
                                                           64 * RT_WFP_CAND_WAVES, lds) != hipSuccess || occ < 1)
            occ = 1;
          c->wfp_occ_lds[shadow ? 1 : 0] = lds;
        }
        g = grid(64 * RT_WFP_CAND_WAVES, ncu * (uint32_t)occ);
        b = dim3(64 * RT_WFP_CAND_WAVES);
      }
      hipLaunchKernelGGL((wfp_cand_kernel<SHADOW, LDS_TRAV>), g, b, lds, st, c->dev, A, P, d, n_ub, n_dev, rows, hc);
    }); });
  };
  // grid-stride evaluations: one pass covers ~4 pairs per ray of the level (fractal: ~3), at most 8 waves per SIMD
  const dim3 ge(std::max<uint32_t>(ncu, std::min<uint32_t>((uint32_t)(((size_t)n_ub * 4 + 63) / 64), ncu * 32u)));
  // the pair counters start at zero with the launch's counter block; the sorts' scratch is zeroed here
  // for the launch's first pair level, by each level's shading kernel for the next
  if (first) RT_HIP(hipMemsetAsync(P.bins, 0, 3 * RT_WFP_BIN_WORDS * 4, st));
  launch_cand(false);
  RT_HIP(rt_wf_bucket_sort(P.key, P.key_s, P.val, P.val_s, P.cap, P.count + WFP_NEAREST, nobj, 0, bins[0], false, st, plan.counted));
  hipLaunchKernelGGL(wfp_near_eval_kernel, ge, b64, 0, st, c->dev, A, P, d, rows);
  hipLaunchKernelGGL(wfp_near_tie_kernel, dim3(std::min<uint32_t>((P.cap + 255) / 256, 4096)), dim3(256), 0, st, P);
  // the hit points and their order for the shadow and shading passes: buckets of (hit object, coarse hit-point cell:
  // WfPlan::cbits), unordered within a bucket (a 16^3-cell-only key and the full 27-bit radix sort measured slower:
  // profiles/r03o_sort_ab.txt, r03w_*; the hit-key kernel counting its keys for this sort, over contiguous 4096-ray
  // chunks, too: 5.63 vs 5.50 ms, profiles/r08a_fractal.txt)
  hipLaunchKernelGGL(wfp_hit_key_kernel, grid(256, ncu * 8), dim3(256), 0, st, c->dev, A, P, d, n_ub, n_dev, rows, plan.cbits);
  if (d < RT_WFP_HITSORT_MAX_D)
    RT_HIP(rt_wf_bucket_sort(P.hkey, P.hkey_s, P.hval, P.hperm, n_ub, n_dev, (nobj + 1u) << plan.cbits, 0, bins[1], false, st));
  else
    P.hperm = P.hval;                     // the level's own order (hval[i] = the i-th ray's slot)
  launch_cand(true);
  RT_HIP(rt_wf_bucket_sort(P.key, P.key_s, P.val, P.val_s, P.cap, P.count + WFP_SHADOW, nobj, 0, bins[2], false, st, plan.counted));
  hipLaunchKernelGGL(wfp_shadow_eval_kernel, ge, b64, 0, st, c->dev, P);
  with_bool(plan.refr, [&](auto R) { with_bool(plan.fc, [&](auto K) {
    hipLaunchKernelGGL((wfp_shade_kernel<decltype(R)::value, decltype(K)::value>), grid(64, ncu * 32), b64, 0, st, c->dev, A, P, d,
                       n_ub, n_dev, rows, plan.max_depth);
  }); });
  RT_HIP(hipGetLastError());
  return RT_OK;
}
