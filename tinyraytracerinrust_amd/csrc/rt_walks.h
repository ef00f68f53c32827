// rt_walks.h -- the second part of the device core (rt_device.h; after rt_core.h): conservative box
// culling in f64 and f32, the hierarchy's node accessors, the oriented-box test, the generic and the
// compile-time-unrolled walk (walk_trav / spec_walk), and the two traversals of raytracer.rs built on
// them: nearest_hit and shadow_transparency.
#pragma once

namespace {

// ------------------------------------------------------------------ conservative culling
// Does the ray segment t in [0, tmax] come near the box?  Only ever answers "no" when no point
// where an accepted hit could lie is on the segment.  Per axis the slab times are
// (bound - o) * inv with inv ~ 1/d to ~1e-15: for |origin|, |bounds| <= 1e6 the error in
// space is < 1e-9, far inside the 1e-6 inflation of every box (scene.cpp leaf_box), so each
// axis interval computed still contains the parameter of any point of the un-inflated region;
// tmax carries a 1e-7 relative margin on top.  min/max are IEEE minNum/maxNum: a NaN slab time
// narrows nothing, and a ray outside the proven range (cull_ray) gets NaN inv -> never culled.
struct CullRay { V3 inv, o; };

// Reciprocal for the culling slabs only (never for a value the reference computes): hardware
// rcp + one Newton step.  d == 0 (or |d| < 1e-200) -> +-1e200, which makes the slab test the
// "origin inside the slab" check while every product stays finite.
__device__ __forceinline__ double cull_rcp(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  const double n = fma(r, fma(-x, r, 1.0), r);
  return fabs(x) < 1e-200 ? copysign(1e200, x) : n;
}
__device__ __forceinline__ CullRay cull_ray(V3 o, V3 d) {
  const double ad = fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z));
  const bool ok = fabs(o.x) <= RT_CULL_COORD_MAX && fabs(o.y) <= RT_CULL_COORD_MAX && fabs(o.z) <= RT_CULL_COORD_MAX &&
                  ad >= 1e-100 && ad <= 1e100;
  const double nan = __builtin_nan("");
  const V3 inv = ok ? V3{cull_rcp(d.x), cull_rcp(d.y), cull_rcp(d.z)} : V3{nan, nan, nan};
  return {inv, o};
}
// (bound - o) * inv per slab: measured faster than fma(bound, inv, -o*inv), which keeps three
// more doubles live across the traversal (profiles/r01n_variant_timing.txt).
template <class P> __device__ __forceinline__ bool box_may_hit(P lo, P hi, const CullRay& r, double tmax) {
  const double ax = (lo[0] - r.o.x) * r.inv.x, bx = (hi[0] - r.o.x) * r.inv.x;
  const double ay = (lo[1] - r.o.y) * r.inv.y, by = (hi[1] - r.o.y) * r.inv.y;
  const double az = (lo[2] - r.o.z) * r.inv.z, bz = (hi[2] - r.o.z) * r.inv.z;
  const double tn = fmax(fmax(fmin(ax, bx), fmin(ay, by)), fmax(fmin(az, bz), 0.0));
  const double tf = fmin(fmin(fmax(ax, bx), fmax(ay, by)), fmin(fmax(az, bz), tmax));
  return !(tn > tf);
}
__device__ __forceinline__ double cull_tmax(double t) { return t * (1.0 + 1e-7) + 1e-7; }

// The same test in f32 (RT_CULL_F32, the traversals of the megakernels and the deferred kernel): half
// the registers of the f64 culling ray, f32 instructions at twice the f64 issue rate, and the box
// bounds as 32-bit literals (VOP2 operands) in the specialised programs.  Conservative by construction:
//  * a ray is culled only if every origin coordinate is within RT_CULL32_COORD_MAX and its largest
//    direction component within [2^-10, 2^10] (cull_ray_f; otherwise every slab time is NaN, which
//    narrows nothing: min/max are IEEE minNum/maxNum);
//  * the f32 boxes are the f64 boxes grown by RT_CULL32_MARGIN = 4x the error of rounding such an origin
//    to f32, then rounded outward (scene.cpp f32_boxes), so the slab times computed from the rounded
//    origin bound those of the exact origin against a box that still contains the f64 box;
//  * what remains is relative: fl32(box - o) * rcp32(fl32(d)) is within 2^-21 of its exact value, and
//    the comparison tn <= tf allows 2^-18 of slack on each side;
//  * a direction component below 2^-100 is taken as zero (inv = +-inf): reaching a slab RT_CULL32_MARGIN
//    away would take t > 2^93, where the largest component (>= 2^-10) has left every box (|bounds| <= 1e6);
//    (box - o) * inf is +-inf, or NaN (narrows nothing) when box - o == 0;
//  * the only infinite time that reaches the comparison is tn = +inf from such a zero component with
//    the origin outside its slab (the ray never enters it: exact), and tf is finite (some component
//    is >= 2^-10), so the slack never hides an infinity.
// Chosen per translation unit: the specialised programs and k_points.hip walk with it, the other
// generic units with the f64 test (fractal.scene's generic walks ran 21 % slower in f32, DESIGN.md
// section 7).
#ifndef RT_CULL_F32
#ifdef RT_SPEC
#define RT_CULL_F32 1
#else
#define RT_CULL_F32 0
#endif
#endif
struct CullRayF { float ix, iy, iz, ox, oy, oz; };   // 1 / d and o (f32)
__device__ __forceinline__ float cull_rcp_f(float x) {
  return fabsf(x) < 0x1p-100f ? copysignf(__builtin_inff(), x) : __builtin_amdgcn_rcpf(x);
}
__device__ __forceinline__ CullRayF cull_ray_f(V3 o, V3 d) {
  const double ad = fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z));
  const bool ok = fabs(o.x) <= RT_CULL32_COORD_MAX && fabs(o.y) <= RT_CULL32_COORD_MAX &&
                  fabs(o.z) <= RT_CULL32_COORD_MAX && ad >= 0x1p-10 && ad <= 0x1p10;
  const float nan = __builtin_nanf("");
  const float ix = ok ? cull_rcp_f((float)d.x) : nan, iy = ok ? cull_rcp_f((float)d.y) : nan,
              iz = ok ? cull_rcp_f((float)d.z) : nan;
  return {ix, iy, iz, (float)o.x, (float)o.y, (float)o.z};
}
template <class P> __device__ __forceinline__ bool fbox_may_hit(P lo, P hi, const CullRayF& r, float tmax) {
  const float ax = (lo[0] - r.ox) * r.ix, bx = (hi[0] - r.ox) * r.ix;
  const float ay = (lo[1] - r.oy) * r.iy, by = (hi[1] - r.oy) * r.iy;
  const float az = (lo[2] - r.oz) * r.iz, bz = (hi[2] - r.oz) * r.iz;
  const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
  const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax));
  return tn * (1.0f - 0x1p-18f) <= __builtin_fmaf(fabsf(tf), 0x1p-18f, tf);
}
__device__ __forceinline__ float cull_tmax_f(double t) { return (float)cull_tmax(t); }
#if RT_CULL_F32
// The traversals' culling ray and tests, f32 (above) or f64 (box_may_hit)
typedef CullRayF CullR;
typedef float CullT;
#define RT_CULL_NEVER() CullRayF{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.0f, 0.0f, 0.0f}
#define RT_CULL_RAY(o, d) cull_ray_f(o, d)
#define RT_CULL_TMAX(t) cull_tmax_f(t)
#define RT_BOX_MAY_HIT(R, lo, hi, cr, tm) fbox_may_hit((R)->f##lo, (R)->f##hi, cr, tm)
#else
typedef CullRay CullR;
typedef double CullT;
#define RT_CULL_NEVER() CullRay{V3{__builtin_nan(""), __builtin_nan(""), __builtin_nan("")}, V3{0.0, 0.0, 0.0}}
#define RT_CULL_RAY(o, d) cull_ray(o, d)
#define RT_CULL_TMAX(t) cull_tmax(t)
#define RT_BOX_MAY_HIT(R, lo, hi, cr, tm) box_may_hit((R)->lo, (R)->hi, cr, tm)
#endif
// Hierarchy node accessors: the walks' lambdas take a node of either form -- RtTrav (the specialised
// programs' constexpr tables, and f64-culling builds) or RtTravC (the generic walks with f32 culling).
__device__ __forceinline__ int node_obj(cptr<RtTrav> T) { return T->obj; }
__device__ __forceinline__ int node_skip(cptr<RtTrav> T) { return T->skip; }
__device__ __forceinline__ int node_cull(cptr<RtTrav> T) { return T->cull; }
__device__ __forceinline__ int node_shadow_skip(cptr<RtTrav> T) { return T->shadow_skip; }
template <class CR, class TM> __device__ __forceinline__ bool node_may_hit(cptr<RtTrav> T, const CR& cr, TM tm) {
  return RT_BOX_MAY_HIT(T, blo, bhi, cr, tm);
}
__device__ __forceinline__ int node_obj(cptr<RtTravC> T) { return T->obj; }
__device__ __forceinline__ int node_skip(cptr<RtTravC> T) { return (int)(T->skip_flags & 0x0fffffffu); }
__device__ __forceinline__ int node_cull(cptr<RtTravC> T) { return (int)((T->skip_flags >> 28) & 3u); }
__device__ __forceinline__ int node_shadow_skip(cptr<RtTravC> T) { return (int)(T->skip_flags >> 30); }
__device__ __forceinline__ bool node_may_hit(cptr<RtTravC> T, const CullRayF& cr, float tm) {
  return fbox_may_hit(T->lo, T->hi, cr, tm);
}

// The range the host proves constant hit filters for (RtLeaf::filter_const): cull_ray's valid range
// (origin within 1e6, largest direction component within [1e-100, 1e100]).
__device__ __forceinline__ bool const_filter_range(V3 o, V3 d) {
  const double ad = fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z));
  return fabs(o.x) <= RT_CULL_COORD_MAX && fabs(o.y) <= RT_CULL_COORD_MAX && fabs(o.z) <= RT_CULL_COORD_MAX &&
         ad >= 1e-100 && ad <= 1e100;
}

// The object's oriented box (RtObject::obb_leaf, scene.cpp obb): may the segment t in [0, tmax]
// meet the leaf-frame box olo/ohi?  The ray is taken to the leaf's frame with the leaves' own
// arithmetic; outside the range the host's margins are proven for (|o| <= 1e6, unit-length
// directions) the answer is yes.  Only the reflection-only kernels take it (OBB = !REFR in the
// walks below).
__device__ __forceinline__ bool obb_may_hit(const DS& S, cptr<RtObject> O, V3 ro, V3 rd, CullT tmax) {
  RT_REC(R, S, leaves, LEAVES, O->obb_leaf);
  const double ad = fmax(fmax(fabs(rd.x), fabs(rd.y)), fabs(rd.z));
  if (!(ad >= 0.25 && ad <= 4.0 && fabs(ro.x) <= 1e6 && fabs(ro.y) <= 1e6 && fabs(ro.z) <= 1e6)) return true;
  const V3 o = xf(R->inv, ro);
  const V3 d = sub(xf(R->inv, rd), ld3(R->inv_o));
  return RT_BOX_MAY_HIT(O, olo, ohi, RT_CULL_RAY(o, d), tmax);   // leaf-frame ray: cull_ray*'s own range checks
}

// ------------------------------------------------------------------ traversal (raytracer.rs)
// Both traversals walk the object hierarchy (RtTrav, pre-order over contiguous draw-order runs)
// wave-coherently: `i` is uniform, a lane that misses a group resumes at its skip index, and the
// wave jumps over a group no lane entered.  walk_trav calls group(T) for a group node (does this
// lane enter it?) and object(T) for an object node the lane reaches.
// RT_SPEC (the scene-specialised programs, spec_text.cpp): the hierarchy is a constexpr table, so the
// walk is unrolled at compile time into nested branches -- every node's fields, every object's and
// leaf's record are constants, and a branch no lane takes is jumped over by the hardware (EXEC = 0),
// exactly the generic walk's skip.
#ifdef RT_SPEC
#define RT_INL __attribute__((always_inline))
template <int N> struct IC { static constexpr int value = N; };
template <int I, int END, class F>
__device__ __forceinline__ void spec_for(F&& f) {
  if constexpr (I < END) {
    f(IC<I>{});
    spec_for<I + 1, END>(f);
  }
}
// (RT_SPEC_FAMILY: a node's obj and skip are shared by every member of the family, spec_text.cpp checks)
// Tile masks (rt_tilemask.h; single-scene programs of reflection-only scenes): `mask` is wave-uniform,
// bit o clear = no ray of this walk can have an accepted hit in object o's box.  A boxed object's node
// is one scalar bit test; a group whose objects are all boxed is skipped when none of their bits is set
// (both sets are compile-time constants).  Unbounded objects ignore the mask.
#ifndef RT_TILE_MASKS
#ifdef RT_SPEC_FAMILY
#define RT_TILE_MASKS 0
#else
#define RT_TILE_MASKS 1
#endif
#endif
// The dispatch-record operands of the masked single-scene kernels (spec_text.cpp writes them into the megakernel's
// and the primary-ray kernel's text; rows_entry below): a program without masks declares none.
#if RT_TILE_MASKS
#define RT_REC_PARAMS , const RtTileRec* __restrict__ recs
#define RT_REC_ARGS , recs
#else
#define RT_REC_PARAMS
#define RT_REC_ARGS
#endif
template <bool SORD> constexpr uint32_t spec_boxed_bits(int b, int e) {     // the boxed objects of nodes [b, e)
  uint32_t m = 0;
  for (int i = b; i < e; ++i) {
    const RtTrav& T = SORD ? rt_spec::STRAV[i] : rt_spec::TRAV[i];
    if (T.obj >= 0 && T.obj < 32 && T.cull == RT_CULL_BOX) m |= 1u << T.obj;
  }
  return m;
}
template <bool SORD> constexpr bool spec_all_boxed(int b, int e) {          // no unbounded object in nodes [b, e)
  for (int i = b; i < e; ++i) {
    const RtTrav& T = SORD ? rt_spec::STRAV[i] : rt_spec::TRAV[i];
    if (T.obj >= 32 || (T.obj >= 0 && T.cull == RT_CULL_NONE)) return false;
  }
  return true;
}
template <bool SORD, int I, int END, class G, class O>
__device__ __forceinline__ void spec_walk(const DS& S, G& group, O& object, uint32_t mask) {
  if constexpr (I < END) {
    constexpr RtTrav T = SORD ? rt_spec::STRAV[I] : rt_spec::TRAV[I];
    auto body = [&](cptr<RtTrav> TP) RT_INL {
      if constexpr (T.obj < 0) {
        constexpr bool GM = RT_TILE_MASKS && spec_all_boxed<SORD>(I + 1, T.skip);
        constexpr uint32_t gbits = spec_boxed_bits<SORD>(I + 1, T.skip);
        if (!GM || (mask & gbits) != 0u)
          if (group(TP)) spec_walk<SORD, I + 1, T.skip>(S, group, object, mask);
        spec_walk<SORD, T.skip, END>(S, group, object, mask);
      } else {
        constexpr bool OM = RT_TILE_MASKS && T.cull == RT_CULL_BOX && T.obj < 32;
        if (!OM || ((mask >> (T.obj & 31)) & 1u) != 0u) object(TP);
        spec_walk<SORD, I + 1, END>(S, group, object, mask);
      }
    };
    if constexpr (SORD) {
      RT_REC(TP, S, strav, STRAV, I);
      body(TP);
    } else {
      RT_REC(TP, S, trav, TRAV, I);
      body(TP);
    }
  }
}
#else
#define RT_INL
#endif
// STOP (the shadow walk's early-out): stop(T) after an object node says whether this lane is done;
// once no lane walks on, the generic walk ends (the spec walk's remaining branches are skipped by
// the hardware, EXEC = 0).
template <bool SORD, bool STOP = false, class G, class O>
__device__ __forceinline__ void walk_trav(const DS& S, G&& group, O&& object, bool* done = nullptr,
                                          uint32_t mask = 0xffffffffu) {
#ifdef RT_SPEC
  spec_walk<SORD, 0, SORD ? rt_spec::N_STRAV : rt_spec::N_TRAV>(S, group, object, mask);
#else
  // f32 culling: the compact nodes (RtTravC: two per scalar-cache line)
#if RT_CULL_F32
  const cptr<RtTravC> TR = SORD ? S.strav_c : S.trav_c;
#else
  const cptr<RtTrav> TR = SORD ? S.strav : S.trav;
#endif
  const int n_tr = SORD ? S.n_strav : S.n_trav;
  int resume = 0;
  for (int i = 0; i < n_tr;) {
    const auto T = &TR[i];
    const bool act = i >= resume;
    if (node_obj(T) < 0) {                               // group node
      const bool in = act && group(T);
      if (act && !in) resume = node_skip(T);
      i = __ballot(in) ? i + 1 : node_skip(T);
      continue;
    }
    ++i;
    if (act) object(T);
    if constexpr (STOP)
      if (__ballot(!*done) == 0) break;
  }
#endif
}

// The culling ray of a walk under a tile mask (spec_walk): a walk whose mask holds none of the scene's
// boxed objects tests no object or group box, so it skips the ray's conversions and reciprocals (a
// wave-uniform branch) and takes the ray that culls nothing (NaN slab times, as out of range): the
// per-leaf boxes of unbounded objects, the only tests left, then always pass.
template <bool SORD> __device__ __forceinline__ CullR walk_cull_ray(V3 o, V3 d, uint32_t mask) {
#if defined(RT_SPEC) && RT_TILE_MASKS
  constexpr uint32_t boxed = spec_boxed_bits<SORD>(0, SORD ? rt_spec::N_STRAV : rt_spec::N_TRAV);
  if ((mask & boxed) == 0u) return RT_CULL_NEVER();
#endif
  return RT_CULL_RAY(o, d);
}

// Nearest hit over all objects in draw order: accept d if d > EPS && d < nearest
// (raytracer.rs:141-150).  The acceptance test is pure, so it runs BEFORE the (pure) CSG
// filter: candidates that cannot win never pay for the sibling is_inside tests.
// SHARE: concentric sphere leaves reuse their ray terms (SphereShare); it keeps three doubles live
// across the leaf loop, so only kernels with register headroom take it (see trace()).
template <bool SHARE = false, bool OBB = !SHARE>
RT_FN int nearest_hit(const DS& S, V3 ro, V3 rd, double* dist, uint32_t mask = 0xffffffffu) {
  double best = INFINITY;
  int bobj = -1;
  SphereShare shr = {0.0, 0.0, 0.0};
  constexpr bool NORDER = OBB;
  const CullR cr = walk_cull_ray<NORDER>(ro, rd, mask);
  const bool cf_ok = SHARE && const_filter_range(ro, rd);
  const bool fin = wave_finite(ro, rd);
  // NORDER (reflection-only kernels): the objects in S.strav's order, largest regions first, so an
  // early hit on a big object culls what lies behind it.  Exact: a candidate equal to the best
  // distance so far wins when its object comes earlier in DRAW order (o < bobj), which is the
  // reference's first-visited-wins rule (raytracer.rs:141-150) for any visiting order.
  auto group = [&](auto T) RT_INL { return node_may_hit(T, cr, RT_CULL_TMAX(best)); };
  auto object = [&](auto T) RT_INL {
    // the object's cull kind and box come from the node's copy (RtTrav): one scalar load for the
    // node decides the common case; the object's own record is read only once its box passes
    if (node_cull(T) == RT_CULL_ALWAYS) return;
    if (node_cull(T) == RT_CULL_BOX && !node_may_hit(T, cr, RT_CULL_TMAX(best))) return;
    const int o = node_obj(T);
    RT_REC(O, S, objects, OBJECTS, o);
    if (OBB && O->obb_leaf >= 0 && !obb_may_hit(S, O, ro, rd, RT_CULL_TMAX(best))) return;
    const int lb = O->leaf_begin, le = lb + O->leaf_count;
    RT_SPEC_UNROLL
    for (int l = lb; l < le; ++l) {
      RT_REC(L, S, leaves, LEAVES, l);
      if (O->leaf_cull) {
        if (L->cull == RT_CULL_ALWAYS) continue;
        if (L->cull == RT_CULL_BOX && !RT_BOX_MAY_HIT(L, blo, bhi, cr, RT_CULL_TMAX(best))) continue;
      }
      double t0 = 0.0, t1 = 0.0;
      int n = leaf_candidates<true>(L, ro, rd, fin, &t0, &t1, SHARE ? &shr : nullptr);
      const bool filtered = L->prog_end != L->prog_begin && !(cf_ok && L->filter_const);
      if (n >= 1 && t0 > EPS && (t0 < best || (NORDER && t0 == best && o < bobj)) &&
          (!filtered || leaf_filter(S, L, add(ro, scale(rd, t0))))) {
        best = t0; bobj = o;
      }
      if (n >= 2 && t1 > EPS && (t1 < best || (NORDER && t1 == best && o < bobj)) &&
          (!filtered || leaf_filter(S, L, add(ro, scale(rd, t1))))) {
        best = t1; bobj = o;
      }
    }
  };
  walk_trav<NORDER>(S, group, object, nullptr, mask);
  *dist = best;
  return bobj;
}

// Product of the transparencies of every filtered hit with EPS < d < dist (raytracer.rs:181-197).
// Early-out once the product is exactly 0 (it stays 0: every factor is finite, checked on the
// host), objects of transparency exactly 1.0 are skipped (x * 1.0 == x).
// SORDER (reflection-only kernels): walk S.strav, the likeliest occluders first (scene.cpp
// shadow_order) -- every transparency is +-0 there, so the first filtered hit decides and the
// order is free.  The early return ends the walk: `done` skips the rest of it (in the generic
// walk a finished lane only rides along; the wave leaves once every lane is done).
template <bool SHARE = false, bool OBB = !SHARE, bool SORDER = OBB>
RT_FN double shadow_transparency(const DS& S, V3 p, V3 dir, double dist, uint32_t mask = 0xffffffffu) {
  RT_OPAQUE(p.x);
  RT_OPAQUE(p.y);
  RT_OPAQUE(p.z);
  double tr = 1.0;
  bool done = false;
  SphereShare shr = {0.0, 0.0, 0.0};
  const CullR cr = walk_cull_ray<SORDER>(p, dir, mask);
  const bool cf_ok = SHARE && const_filter_range(p, dir);
  const bool fin = wave_finite(p, dir);
  const CullT tmax = RT_CULL_TMAX(dist);
  auto group = [&](auto T) RT_INL { return !done && node_may_hit(T, cr, tmax); };
  auto object = [&](auto T) RT_INL {
    if (done) return;
    if (node_shadow_skip(T) || node_cull(T) == RT_CULL_ALWAYS) return;   // the node's copies (see nearest_hit)
    if (node_cull(T) == RT_CULL_BOX && !node_may_hit(T, cr, tmax)) return;
    RT_REC(O, S, objects, OBJECTS, node_obj(T));
    if (OBB && O->obb_leaf >= 0 && !obb_may_hit(S, O, p, dir, tmax)) return;
    const double tobj = O->transparency;
    const int lb = O->leaf_begin, le = lb + O->leaf_count;
    RT_SPEC_UNROLL
    for (int l = lb; l < le; ++l) {
      RT_REC(L, S, leaves, LEAVES, l);
      if (O->leaf_cull) {
        if (L->cull == RT_CULL_ALWAYS) continue;
        if (L->cull == RT_CULL_BOX && !RT_BOX_MAY_HIT(L, blo, bhi, cr, tmax)) continue;
      }
      double t0 = 0.0, t1 = 0.0;
      int n = leaf_candidates<true>(L, p, dir, fin, &t0, &t1, SHARE ? &shr : nullptr);
      const bool filtered = L->prog_end != L->prog_begin && !(cf_ok && L->filter_const);
      if (n >= 1 && t0 > EPS && t0 < dist && (!filtered || leaf_filter(S, L, add(p, scale(dir, t0))))) {
        tr *= tobj;
        if (tr == 0.0 && S.shadow_early_out) { done = true; return; }
      }
      if (n >= 2 && t1 > EPS && t1 < dist && (!filtered || leaf_filter(S, L, add(p, scale(dir, t1))))) {
        tr *= tobj;
        if (tr == 0.0 && S.shadow_early_out) { done = true; return; }
      }
    }
  };
  walk_trav<SORDER, true>(S, group, object, &done, mask);
  return done ? 0.0 : tr;
}

}  // namespace
