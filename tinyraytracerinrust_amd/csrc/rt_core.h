// rt_core.h -- the first part of the device core (rt_device.h, which every unit includes instead): the
// correctly rounded sqrt / division cores, the scene's device view (DS, RT_REC), vector and colour
// helpers, the primitives (math_shapes.rs), sphere UV with its texel guard, a leaf's candidate hit
// distances and the CSG hit filter.
#pragma once
#define RT_HD __device__
#include "rt_blob.h"

// Correctly rounded sqrt(x) and 1/sqrt-derived reciprocals without their range handling.
// For f64 `sqrt` and `/` the compiler emits (gfx950) scaled Newton sequences:
//   sqrt(x): x scaled by 2^256 if x < 2^-767, y = rsq(x), g = x*y, h = 0.5*y, r = fma(-h,g,0.5),
//            g = fma(g,r,g), h = fma(h,r,h), twice {d = fma(-g,g,x), g = fma(d,h,g)}, g scaled back,
//            and x itself returned for +-0 / +inf (17 VALU instructions);
//   a / b:   v_div_scale of b and of a, rcp, 4 Newton fmas, mul, fma, v_div_fmas, v_div_fixup (11).
// For x in [2^-767, DBL_MAX] the scalings are by 2^0 and the class select returns g, so the
// unscaled core below is the SAME operation sequence on the same values: bit-identical.  Then
// l = sqrt(x) is in [2^-383.5, 2^512): for 1.0 / l v_div_scale scales neither operand (both
// normal, exponent gap < 768, 1/l and the quotient normal), so v_div_fmas is a plain fma (VCC 0),
// the mul by the numerator 1.0 is exact, and v_div_fixup returns its positive normal operand:
// again the same values.  The range test is wave-uniform (one ballot), outside it the compiler's
// sequences run.
static __device__ __forceinline__ double sqrt_core(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, x);
  return __builtin_fma(d, h, g);
}
static __device__ __forceinline__ double recip_core(double l) {     // 1.0 / l for l in [2^-384, 2^512]
  const double nl = -l;
  const double r = __builtin_amdgcn_rcp(l);
  const double f0 = __builtin_fma(nl, r, 1.0);
  const double f1 = __builtin_fma(r, f0, r);
  const double f2 = __builtin_fma(nl, f1, 1.0);
  const double f3 = __builtin_fma(f1, f2, f1);
  const double f4 = __builtin_fma(nl, f3, 1.0);            // mul = 1.0 * f3 = f3
  return __builtin_fma(f4, f3, f3);
}
// a / b when neither v_div_scale scales (both operands normal, exponent gap < 768, quotient
// normal, |a| >= 2^-969) or a == 0: the compiler's sequence with those identities dropped;
// v_div_fixup is kept, so a zero numerator gives the same signed zero.
static __device__ __forceinline__ double div_core(double a, double b) {
  const double nb = -b;
  const double r = __builtin_amdgcn_rcp(b);
  const double f0 = __builtin_fma(nb, r, 1.0);
  const double f1 = __builtin_fma(r, f0, r);
  const double f2 = __builtin_fma(nb, f1, 1.0);
  const double f3 = __builtin_fma(f1, f2, f1);
  const double m = a * f3;
  const double f4 = __builtin_fma(nb, m, a);
  return __builtin_amdgcn_div_fixup(__builtin_fma(f4, f3, m), b, a);
}
// rt_math.h's rt_acos takes these for the operations whose operand ranges it guarantees.
#define RT_SQRT_IN_RANGE(x) sqrt_core(x)
#define RT_DIV_IN_RANGE(a, b) div_core(a, b)
#include "rt_math.h"

// The device functions below are inlined into every kernel.  In the specialised program (RT_SPEC,
// one module holding 8 kernels of one scene) the inliner would otherwise keep the big ones as
// calls (14 s_swappc, the call ABI's saves and scratch); every kernel instantiates its own copy.
#ifdef RT_SPEC
// A value the optimiser must treat as computed here: trace()'s light loop calls the shadow walk with
// the same origin for every light (and the shading inputs once, inside the loop), and with every box
// and transform a constant the terms on the hit point ((lo - o), xf(inv, o), every object's CSG
// inside / on-surface tests) become loop-invariant -- LICM hoists (speculates) those of EVERY box,
// leaf and object out of the light loop and the spec kernel spills ~200 VGPRs.  Re-defining the point
// where it is used keeps each term where the generic kernel computes it (no instruction, no value
// change).
#define RT_OPAQUE(x) asm volatile("" : "+v"(x))
#define RT_FN __device__ __attribute__((always_inline))
#define RT_SPEC_UNROLL _Pragma("unroll")   // loops over a constant record's runs: unroll them fully
#else
#define RT_OPAQUE(x) (void)0
#define RT_FN __device__
#define RT_SPEC_UNROLL
#endif

namespace {

// Scene tables are read-only for the whole launch: view them through the CONSTANT address space
// (4) so uniform-index reads compile to scalar (SMEM) loads instead of per-lane VMEM loads.
// A family program (RT_SPEC_FAMILY) reads its tables through generic pointers (fam_rec).
#if defined(RT_SPEC_FAMILY)
#define CAS
#else
#define CAS __attribute__((address_space(4)))
#endif
template <class T> using cptr = const CAS T*;
template <class T> __device__ __forceinline__ cptr<T> as_const(const T* p) { return (cptr<T>)p; }

// Record I of scene table `tab` (objects, trav, strav, leaves, lights) as `cptr<T> NAME`.
// RT_SPEC_FAMILY (spec_text.cpp: ONE program for a family of scenes of the same structure -- the frames of
// an animation): the record is assembled word by word, the 4-byte words every member of the family
// shares from the program's constexpr table (they fold like the single-scene program's), the words
// that differ between members from this scene's table in HBM (scalar loads).  The table stays
// exactly the scene's own: the merge only decides which words the compiler may treat as constants.
#ifdef RT_SPEC_FAMILY
template <class T> struct FamRec { T v; };
template <class T, int N>
__device__ __forceinline__ FamRec<T> fam_rec(const T (&ct)[N], const uint8_t* vary, const T* rt, int i) {
  constexpr int NW = (int)(sizeof(T) / 4);
  const uint32_t* cw = (const uint32_t*)(const void*)&ct[i];
  const __attribute__((address_space(4))) uint32_t* rw =
      (const __attribute__((address_space(4))) uint32_t*)(const void*)rt + (size_t)i * NW;
  uint32_t w[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) w[k] = vary[i * NW + k] ? rw[k] : cw[k];
  return FamRec<T>{__builtin_bit_cast(T, w)};
}
#define RT_REC(NAME, S, tab, TAB, I)                                                   \
  const auto NAME##_rec = fam_rec(rt_spec::TAB, rt_spec::VARY_##TAB, (S).tab, (I)); \
  const auto NAME = &NAME##_rec.v
#else
#define RT_REC(NAME, S, tab, TAB, I) const auto NAME = &(S).tab[I]
#endif

struct DS {                         // device view of RtDevScene
  cptr<RtObject> objects;
  cptr<RtTrav> trav;
  cptr<RtTrav> strav;               // shadow-ray walk of scenes without a transparent object
  cptr<RtTravC> trav_c;             // the same, compact (the generic walks with f32 culling)
  cptr<RtTravC> strav_c;
  cptr<RtNode> nodes;
  cptr<RtLeaf> leaves;
  cptr<RtProg> prog;
  cptr<RtLight> lights;
  cptr<RtTexture> textures;
  const uint8_t* texels;            // per-lane texel gathers stay global (vector) loads
  int n_objects, n_lights, n_trav, n_strav;
  int shadow_early_out;
};

constexpr double EPS = RT_EPSILON;
constexpr double PI_D = 3.14159265358979323846;   // std::f64::consts::PI

struct V3 { double x, y, z; };
struct Col { double r, g, b; };

__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ bool wave_sqrt_core_ok(double x) {
  return __ballot(!(x >= 0x1p-767 && x <= 0x1.fffffffffffffp+1023)) == 0;
}
__device__ __forceinline__ double sqrt_rt(double x) {
  if (wave_sqrt_core_ok(x)) return sqrt_core(x);
  return sqrt(x);
}
__device__ __forceinline__ double len(V3 a) { return sqrt_rt(dot(a, a)); }
// l = len(a) and il = 1.0 / l, as `len(a)` and `1.0 / len(a)` compute them
__device__ __forceinline__ void len_inv(V3 a, double* l, double* il) {
  const double x = dot(a, a);
  if (wave_sqrt_core_ok(x)) {
    *l = sqrt_core(x);
    *il = recip_core(*l);
    return;
  }
  *l = sqrt(x);
  *il = 1.0 / *l;
}
__device__ __forceinline__ V3 normalized(V3 a) {
  double l, il;
  len_inv(a, &l, &il);
  return scale(a, il);
}
template <class P> __device__ __forceinline__ V3 ld3(P p) { return {p[0], p[1], p[2]}; }
// transform_vector (transformation.rs:53-59) with rows m[0..3], m[4..7], m[8..11]
template <class P> __device__ __forceinline__ V3 xf(P m, V3 v) {
  return {m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3],
          m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7],
          m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11]};
}
// transform_vector by a diagonal-affine matrix (RtLeaf::xdiag): bit-identical to xf() for finite
// inputs (rt_blob.h), 6 flops instead of 18.
template <class P> __device__ __forceinline__ V3 xf_diag(P m, V3 v) {
  return {m[0] * v.x + m[3], m[5] * v.y + m[7], m[10] * v.z + m[11]};
}
__device__ __forceinline__ bool finite3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
// Is every active lane's vector finite?  Wave-uniform, so the short transform is a scalar branch.
__device__ __forceinline__ bool wave_finite(V3 a) { return __ballot(!finite3(a)) == 0; }
__device__ __forceinline__ bool wave_finite(V3 a, V3 b) { return __ballot(!(finite3(a) && finite3(b))) == 0; }
// The leaf's inverse transform of a point (transformation.rs:53-59); `fin` = wave_finite(v).
__device__ __forceinline__ V3 leaf_inv_xf(cptr<RtLeaf> L, V3 v, bool fin) {
  if (L->xdiag == RT_XF_IDENTITY && fin) return v;
  if (L->xdiag && fin) return xf_diag(L->inv, v);
  return xf(L->inv, v);
}

// color.rs:36-53: clamp each channel (NaN passes through)
// FC (fast clamp): the same clamp as two min/max instructions instead of two compares and four
// selects.  fmin(fmax(x, 0), 1) equals `x < 0 ? 0 : (x > 1 ? 1 : x)` bit for bit for every x
// except NaN (maxNum drops it) and -0 (max(-0, +0) is +0).  The host sets RtDevScene::colour_fast
// only when no colour-op operand can be NaN, negative or -0 (every material / light colour channel
// finite and >= +0, every reflectivity and transparency finite in [0, 1]: then every factor of
// every colour op is finite and >= +0, see rt::flatten), and the kernels take FC = true only then.
// 3.4 % faster on 4K globes, 2 % on spinning_globes (profiles/r02ab.txt).
template <bool FC = false> __device__ __forceinline__ double in_limit(double x) {
  if constexpr (FC) return __builtin_fmin(__builtin_fmax(x, 0.0), 1.0);
  else return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
}
template <bool FC = false> __device__ __forceinline__ Col in_range(double r, double g, double b) {
  return {in_limit<FC>(r), in_limit<FC>(g), in_limit<FC>(b)};
}
template <bool FC = false> __device__ __forceinline__ Col intensify(Col c, double k) { return in_range<FC>(c.r * k, c.g * k, c.b * k); }
template <bool FC = false> __device__ __forceinline__ Col cmul(Col a, Col b) { return in_range<FC>(a.r * b.r, a.g * b.g, a.b * b.b); }
template <bool FC = false> __device__ __forceinline__ Col cadd(Col a, Col b) { return in_range<FC>(a.r + b.r, a.g + b.g, a.b + b.b); }
// `(c * 255.0) as u8` (easy_pixbuf.rs:49-52): saturating truncation, NaN -> 0
__device__ __forceinline__ uint32_t to_u8(double c) {
  double v = c * 255.0;
  if (!(v > 0.0)) return 0u;
  if (v >= 255.0) return 255u;
  return (uint32_t)v;
}

// ------------------------------------------------------------------ primitives (math_shapes.rs)
template <class P> __device__ __forceinline__ bool on_plane(P pl, V3 q) {        // :162-164
  return fabs(pl[0] * q.x + pl[1] * q.y + pl[2] * q.z + pl[3]) < EPS;
}

RT_FN bool leaf_inside(cptr<RtLeaf> L, V3 p, bool fin) {
  int k = L->kind;
  if (k == RT_N_PLANE) return false;                                        // :186-188
  V3 q = leaf_inv_xf(L, p, fin);
  if (k == RT_N_SPHERE) return len(sub(q, ld3(L->c))) <= L->r_eps;         // :70-74
  return q.x <= L->hi[0] && q.x >= L->lo[0] && q.y <= L->hi[1] &&          // :319-328
         q.y >= L->lo[1] && q.z <= L->hi[2] && q.z >= L->lo[2];
}

RT_FN bool leaf_on_surface(cptr<RtLeaf> L, V3 p, bool fin) {
  V3 q = leaf_inv_xf(L, p, fin);
  int k = L->kind;
  if (k == RT_N_SPHERE) return fabs(len(sub(q, ld3(L->c))) - L->radius) < EPS;   // :76-80
  if (k == RT_N_PLANE) return on_plane(L->pl[0], q);                            // :190-194
  bool bx = L->lo_e[0] <= q.x && q.x <= L->hi_e[0];                              // :330-355
  bool by = L->lo_e[1] <= q.y && q.y <= L->hi_e[1];
  bool bz = L->lo_e[2] <= q.z && q.z <= L->hi_e[2];
  if (by && bx && (on_plane(L->pl[0], q) || on_plane(L->pl[5], q))) return true;
  if (bz && bx && (on_plane(L->pl[1], q) || on_plane(L->pl[4], q))) return true;
  if (by && bz && (on_plane(L->pl[2], q) || on_plane(L->pl[3], q))) return true;
  return false;
}

RT_FN V3 leaf_normal(cptr<RtLeaf> L, V3 p, bool fin) {
  int k = L->kind;
  if (k == RT_N_PLANE) return ld3(L->pn[0]);                               // :182-184
  V3 q = leaf_inv_xf(L, p, fin);
  if (k == RT_N_SPHERE) {                                                  // :64-68
    V3 n = sub(q, ld3(L->c));
    return normalized(sub(xf(L->mat, n), ld3(L->mat_o)));
  }
  RT_SPEC_UNROLL
  for (int i = 0; i < 6; ++i)                                              // :292-317
    if (on_plane(L->pl[i], q)) return ld3(L->pn[i]);
  return {1.0, 1.0, 1.0};
}

// MathSphere::get_uv_coordinates (:82-114): the centre is subtracted BEFORE the inverse transform.
// tw, th > 0 (a textured object's texture size): the texel-boundary guard.  The texture lookup truncates
// x = u (tw - 1) and y = th - v (th - 1) - 1 (texture.rs:27-34), and u, v come from two acos and a sin that
// may differ from glibc's (the reference's libm) by an ulp (rt_acos, ocml's sin).  From those ulps the
// guard bounds how far the lane's x and y can be from glibc's (through sin's slope at phi, acos's slope
// 1 / sqrt(1 - r^2) at r, and every rounding on the way, times 16); a lane whose x or y lies within that
// bound of an integer (or of a clamp edge, or whose r is near +-1 or not finite) evaluates phi, sin(phi)
// and theta again with the correctly rounded rt_acos_cr / rt_sin_cr (rt_math.h) -- glibc's values except
// where glibc itself is not correctly rounded.  Far from a boundary both sides truncate to the same texel,
// and the guard costs ~30 flops per textured hit; a 4K frame has ~1e-12 of its hits near a boundary.
// The rare lanes' recomputation.  The specialised programs inline it (their guard costs 0.4 %); the
// generic kernels call it: inlined at each of their shading sites, its double-double code made the
// generic 4K frame 3.6x slower (0.430 -> 1.554 ms, profiles/r09v_generic_ab.txt).
#ifdef RT_SPEC
#define RT_TEXEL_CR_FN __device__ __forceinline__
#else
#define RT_TEXEL_CR_FN __device__ __attribute__((noinline))
#endif
RT_TEXEL_CR_FN void sphere_uv_cr(double cy, double cz, bool flip, double* u, double* v) {
  double phi = rt_acos_cr(cy);                                             // rt_math.h
  if (isnan(phi)) phi = 0.0;
  double theta = rt_acos_cr(cz / rt_sin_cr(phi)) / (2.0 * PI_D);
  if (isnan(theta)) theta = 0.0;
  *v = phi / PI_D;
  *u = flip ? 1.0 - theta : theta;
}
__device__ __forceinline__ double ulp_bound(double a) { return fabs(a) * 0x1p-52 + 0x1p-1074; }
__device__ __forceinline__ bool near_int(double a, double m) { return !(fabs(a - rint(a)) > m); }   // NaN: near
RT_FN void sphere_uv(cptr<RtLeaf> L, V3 p, double* u, double* v, int tw = 0, int th = 0) {
  V3 q = xf(L->inv, sub(p, ld3(L->c)));           // per shaded hit only: no short form
  q = scale(normalized(q), 1.0 - EPS);
  const double cy = -((0.0 * q.x + 1.0 * q.y) + 0.0 * q.z);                  // up = (0,1,0)
  const double cz = (q.x * 0.0 + q.y * 0.0) + q.z * -1.0;                    // u_zero = (0,0,-1)
  const bool flip = (-1.0 * q.x + 0.0 * q.y) + 0.0 * q.z > 0.0;              // u_qrtr = (-1,0,0)
  double phi = rt_acos(cy);
  if (isnan(phi)) phi = 0.0;
  const double sp = sin(phi), r = cz / sp, ac = rt_acos(r);
  double theta = ac / (2.0 * PI_D);
  if (isnan(theta)) theta = 0.0;
  *v = phi / PI_D;
  *u = flip ? 1.0 - theta : theta;
  if (tw > 0) {
    const double x = *u * (double)(tw - 1), y = (double)th - (*v * (double)(th - 1)) - 1.0;
    const double ey = (double)(th - 1) * (2.0 * ulp_bound(phi) / PI_D + ulp_bound(*v)) + 2.0 * ulp_bound(y);
    const double er = 0x1p-50 + 4.0 * ulp_bound(phi) / fabs(sp);
    const double ea = fabs(r) * er / sqrt(fmax(1.0 - r * r, 0x1p-60)) + 2.0 * ulp_bound(ac);
    const double ex = (double)(tw - 1) * (ea / (2.0 * PI_D) + 2.0 * ulp_bound(*u)) + 2.0 * ulp_bound(x);
    if (!(fabs(r) < 1.0 - 0x1p-26) || near_int(x, 16.0 * ex) || near_int(y, 16.0 * ey))
      sphere_uv_cr(cy, cz, flip, u, v);                                      // the rare lanes
  }
}

// Candidate hit distances of one primitive for the world ray (ro, rd):
// RTObject::intersects (rt_object.rs:28-31) = reverse_transform_ray + MathShape::intersects.
// `fin` = wave_finite(ro, rd): selects the exact short forms for identity / diagonal-affine
// leaves (rt_blob.h).  POS: the caller accepts only t > EPS (the traversals), so a plane whose
// distance is provably <= 0 from the signs alone skips its division (see the plane branch).
// SphereShare: a traversal's per-lane record of the last sphere leaf's ray terms.  A sphere leaf
// with RtLeaf::share_prev (the previous leaf of its object is a sphere with a bit-identical
// inverse transform and centre, and is evaluated by every lane that evaluates this one, see
// rt_blob.h) has the same object-space ray, hence the same 1/|d|, v.dn and v.v: only r^2 differs,
// so it reuses them and skips the transform, the length, the division and two dot products.
struct SphereShare { double il, vd, vv; };

template <bool POS = false>
__device__ __forceinline__ int leaf_candidates(cptr<RtLeaf> L, V3 ro, V3 rd, bool fin, double* t0, double* t1,
                                               SphereShare* sh = nullptr) {
  if (sh && L->share_prev) {                                               // math_shapes.rs:42-62
    const double sum = sh->vd * sh->vd - (sh->vv - L->r2);
    if (sum < 0.0) return 0;
    const double sq = sqrt_rt(sum);
    *t0 = (-sh->vd + sq) * sh->il;
    *t1 = (-sh->vd - sq) * sh->il;
    return 2;
  }
  V3 o, d;
  if (L->xdiag == RT_XF_IDENTITY && fin) {
    o = ro;
    d = rd;
  } else if (L->xdiag && fin) {                                            // transformation.rs:88-93
    o = xf_diag(L->inv, ro);
    d = sub(xf_diag(L->inv, rd), ld3(L->inv_o));
  } else {
    o = xf(L->inv, ro);
    d = sub(xf(L->inv, rd), ld3(L->inv_o));
  }
  int k = L->kind;
  if (k == RT_N_SPHERE) {                                                  // math_shapes.rs:42-62
    V3 v = sub(o, ld3(L->c));
    double l, il;
    len_inv(d, &l, &il);                                                   // il = 1.0 / len(d)
    V3 dn = scale(d, il);
    double vd = dot(v, dn);
    const double vv = dot(v, v);
    if (sh) *sh = {il, vd, vv};
    double sum = vd * vd - (vv - L->r2);
    if (sum < 0.0) return 0;
    double sq = sqrt_rt(sum);
    *t0 = (-vd + sq) * il;
    *t1 = (-vd - sq) * il;
    return 2;
  }
  if (k == RT_N_PLANE) {                                                   // :168-180
    V3 pn = ld3(L->pnorm);
    double v_d, num;
    const int ax = L->plane_axis;
    if (POS && fin && ax >= 0) {               // axis-aligned normal: one product (rt_blob.h)
      if (ax == 0) { v_d = pn.x * d.x; num = pn.x * o.x; }
      else if (ax == 1) { v_d = pn.y * d.y; num = pn.y * o.y; }
      else { v_d = pn.z * d.z; num = pn.z * o.z; }
    } else {
      v_d = dot(pn, d);
      num = dot(pn, o);
    }
    if (v_d != 0.0) {
      num = num + L->pl[0][3];
      // t = -num * (1/v_d) is > 0 only if num and v_d have opposite signs (rounding keeps signs;
      // 1/v_d may overflow to +-inf, never to 0).  Otherwise t is <= 0, -0 or NaN: never > EPS.
      if (POS && !((num > 0.0 && v_d < 0.0) || (num < 0.0 && v_d > 0.0))) return 0;
      // |t| <= |num| / |v_d| (1 + 2^-52)^2 < EPS when |num| <= 2^-22 |v_d| (the product is exact or
      // rounds towards 0): never accepted.  A ray leaving the plane it starts on (the floor's shadow and
      // reflection rays) skips the division.
      if (POS && fabs(num) <= 0x1p-22 * fabs(v_d)) return 0;
      double t = -num * (1.0 / v_d);
      if (t >= 0.0) { *t0 = t; return 1; }
    }
    return 0;
  }
  double tn = -INFINITY, tf = INFINITY;                                    // :248-290
#define RT_SLAB(P, D, I)                                                    \
  if (D == 0.0) {                                                           \
    if (P < L->lo[I] || P > L->hi[I]) return 0;                             \
  } else {                                                                  \
    double a = (L->lo[I] - P) / D, b = (L->hi[I] - P) / D;                  \
    if (a > b) { double tmp = a; a = b; b = tmp; }                          \
    if (a > tn) tn = a;                                                     \
    if (b < tf) tf = b;                                                     \
    if (tn > tf || tf < 0.0) return 0;                                      \
  }
  RT_SLAB(o.x, d.x, 0)
  RT_SLAB(o.y, d.y, 1)
  RT_SLAB(o.z, d.z, 2)
#undef RT_SLAB
  *t0 = tn;
  *t1 = tf;
  return 2;
}

// Conjunction of every CSG ancestor's sibling test for a hit of leaf L at world point p
// (csg.rs:43-95), as a postfix program over a bit stack.
RT_FN bool leaf_filter(const DS& S, cptr<RtLeaf> L, V3 p) {
  const bool fin = wave_finite(p);
  const int nl = L->n_lit;
  if (nl >= 0) {                                   // conjunction of literals (rt_blob.h)
    RT_SPEC_UNROLL
    for (int k = 0; k < nl; ++k) {
      const int v = L->lit[k];
      RT_REC(LI, S, leaves, LEAVES, v >> 1);
      if (leaf_inside(LI, p, fin) != (bool)(v & 1)) return false;
    }
    return true;
  }
  uint32_t st = 0;
  const int e = L->prog_end;
  RT_SPEC_UNROLL
  for (int k = L->prog_begin; k < e; ++k) {
    const int op = S.prog[k].op, arg = S.prog[k].arg;
    if (op == RT_OP_INSIDE) {
      RT_REC(LI, S, leaves, LEAVES, arg);
      st = (st << 1) | (leaf_inside(LI, p, fin) ? 1u : 0u);
    } else if (op == RT_OP_REQUIRE) {
      uint32_t v = st & 1u;
      st >>= 1;
      if (v != (uint32_t)arg) return false;
    } else {
      uint32_t b = st & 1u;
      st >>= 1;
      uint32_t a = st & 1u, r;
      if (op == RT_OP_AND) r = a & b;
      else if (op == RT_OP_OR) r = a | b;
      else r = a & (b ^ 1u);
      st = (st & ~1u) | r;
    }
  }
  return true;
}

}  // namespace
