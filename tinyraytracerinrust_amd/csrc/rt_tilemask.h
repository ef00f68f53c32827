// rt_tilemask.h -- per-tile object masks: which objects a wave's rays can possibly hit, decided once
// per upload and launch geometry instead of once per ray (DESIGN.md "Tile masks").
//
// A wave of the row kernels renders one RT_TILE_W x RT_TILE_H pixel tile.  Its primary rays share an
// origin and fill a fixed cone; where the whole tile lands on one plane (the floor), its shadow rays to
// light l fill a fixed pyramid with apex at the light, and its reflection rays a fixed cone from the
// camera mirrored in the plane.  Whether each of those volumes can touch an object's box is the same
// for all 64 lanes and for every frame of an upload, so this predicate answers it per tile (host and
// device, plain f64 C++, no contraction) and the specialised row kernels test one scalar bit per object
// instead of the lanes' box tests (rt_device.h spec_walk).
//
// Per tile RT_TILEMASK_WORDS 32-bit words: prim, shadow[0..3], refl; bit o = object o (the specialised
// programs have at most 32 objects); a word the predicate computed holds no bit beyond the scene's
// objects, a word it gave up on is 0xffffffff.  A bit may be 0 ONLY IF no ray of that class from any
// pixel of the tile can have an accepted hit of object o, all of which lie inside its culling box
// blo/bhi and inside every further bound below -- then skipping the object changes no accepted hit, and
// the pixels are bit-identical.  Objects without a finite box keep their bit (but for the mask plane's
// own bit in `prim`, see below).
//
// Why a cleared bit is safe (the argument, in the style of the f32-culling comment in rt_device.h):
//  * camera_ray is LINEAR in (sx, sy) and not normalised, so the primary rays of the tile's pixels
//    [x0, x1] x [y0, y1] lie in the cone from cam.center spanned by the four directions at the corners
//    of that rectangle.  The predicate takes the rectangle GROWN BY HALF A PIXEL on every side: every
//    real ray is then at least half a pixel inside every side plane of the cone, an angular slack of
//    >= 0.5 / max(W, H) of the field of view (>= 7.6e-6 for frames up to 65 536 pixels wide).
//  * every rounding involved is relative 2^-52 per operation: the corner directions (3 operations), the
//    side-plane normals (a cross product whose cancellation is bounded by the tile's angular width,
//    8 pixels: relative error <= 2^-52 W / 8 < 2^-39), the corner dot products (the test leaves
//    1e-12 of their magnitude as tolerance), and on the kernel's side the hit point p = ro + rd t
//    (a few ulp of |p| <= 1e6: < 1e-9 in space) and the reflected direction (3 ulp).  All of them
//    together move a ray by < 1e-9 relative, four orders of magnitude inside the half-pixel slack; and
//    every culling box is inflated by >= 1e-6 (scene.cpp leaf_box) beyond the region of accepted hits,
//    which covers the absolute 1e-9 of the hit point.
//  * the mask plane (the first object in draw order that is one plane leaf with RtObject::unit_normal)
//    is taken in world space from the leaf's inverse transform, the form leaf_candidates evaluates.
//    Q = the four points where the grown corner rays meet it.  Plane hits of the tile's rays lie in
//    conv(Q) (a projective image of the rectangle: convex while every corner ray meets the plane at
//    t > 0).  A corner ray must meet the plane at an angle of cosine >= 1e-4 to the normal: the hit
//    parameter's relative error is 2^-52 / cosine <= 2.3e-12, again far inside the slack; a tile with
//    the horizon inside (some corner ray parallel to or leaving the plane) is all ones.
//  * shadow[l]: the shadow rays of those hits are the segments from conv(Q) to L, inside the pyramid
//    conv(Q u {L}).  An object is out when its 8 box corners are all outside one of the four planes
//    through L and an edge of Q, all on the far side of the mask plane from L, all beyond the plane
//    through L parallel to the mask plane, or its box is disjoint from the AABB of Q u {L}.  The
//    pyramid is bounded, so a box rising above the light needs no special case -- but a side plane is an
//    infinite plane through L, and a box that rises above L crosses it beyond the apex, at any distance
//    to the side.  The pyramid lies on the floor's side of the plane through L parallel to the mask
//    plane, so the side planes are asked only about the part of each bound on that side (tm_clip_outside:
//    the corners inside and the points where edges cross, a convex polytope's vertices; its comment has
//    the tolerances: corners 1e-12, crossing points 1e-7 of the dot product's magnitude, the clip itself
//    only ever looser).  Nothing left on that side: out.
//  * vertex sets (k_masks.hip object_bounds): beside the world box an object has up to
//    RT_TILEMASK_OBJ_SETS sets of 8 world-space corners, one per leaf R that scene.cpp obb() accepts as
//    required (R is a sphere or cube and every other leaf's filter holds the literal 2R+1: a hit of R
//    lies on R, any other accepted hit passed R's is_inside; rt::required_leaf_box is obb()'s own test).
//    Each is R's box in R's frame with obb()'s margins (>= 1e-6 (1 + |M_i| + |T_i|) per axis, a hundred
//    times the rounding of q = M p + b for |p| <= 1e6), cut to the extent the other required leaves'
//    corners have in that frame (hits lie in all of those hulls; every cut face is moved out again by the
//    same margin), and taken to world space through the inverse of R.inv computed in long double.  A
//    corner is kept only if R.inv takes it back to its local point within a quarter of the margin, so
//    the hull of the 8 holds the local box with three quarters of it; a singular or non-finite
//    transform, or a corner beyond RT_CULL_COORD_MAX, drops the set.  The corners form an affine image of
//    a box, so corner k's edge neighbours are k^1, k^2, k^4 (rounding bends a face by < 1e-15 relative,
//    inside every tolerance).  An object is outside a half-space when ANY of its bounds is wholly
//    outside, since every bound holds all accepted hits; the world box is tried first.
//  * ball: a required sphere leaf whose transform is a similarity (M M^T = s^2 I within 1e-9) bounds the
//    hits by the world ball |p - centre| <= r_eps / s.  The radius takes obb()'s margin, 1e-6 relative
//    (a thousand times the similarity's tolerance) and 1e-6 (1 + |centre|) absolute; the centre passes
//    the same round trip as a corner.  One ball per object, the smallest.  Outside: the centre's signed
//    distance below -radius, compared as squares with 1e-9 to spare (tm_ball_outside).  At the shadow
//    side planes the ball is clipped at the light too (tm_ball_outside_clipped: the largest value of a
//    linear function over a ball cut by a plane, in closed form; its comment has the cases).
//  * refl: reflect_dir mirrors the direction in the plane's unit normal, so the reflection ray of a hit
//    p is the ray from the mirrored camera centre C' through p, beyond p.  An object is out when its
//    bounds are outside one side plane through C' and an edge of Q, or on C's far side of the plane
//    (not clipped: a clip at the mask plane would cut nothing off objects that stand on the floor).
//    Taken only when RtObject::nunit is parallel to the world plane's normal within 1e-12 (the reference
//    builds a transformed normal separately from the inverse; a rotation's "inverse" is not a true one):
//    otherwise all ones.
//  * everything above is proven for |coordinates| <= RT_CULL_COORD_MAX (camera, lights, boxes, sets, Q) and
//    frames up to 65 536 pixels a side.  Outside that range, with a non-finite value anywhere, more
//    than 4 lights, no mask plane, or a cone whose corner directions are not in convex position (a
//    degenerate camera; the only camera type of this renderer is the perspective one), the class is
//    ALL ONES.  Every comparison is written so that a NaN answers "keep".
//  * which walk takes which word is the kernel's side: rt_device.h trace().
#pragma once
#ifndef __HIPCC_RTC__
#include <math.h>
#include <stdint.h>
#endif
#include "rt_blob.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_TM_HD __host__ __device__ inline
#else
#define RT_TM_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RT_TILEMASK_LIGHTS 4
#define RT_TILEMASK_OBJECTS 32
#define RT_TILEMASK_MAX_SIDE 65536
#define RT_TILEMASK_OBJ_SETS 4       // vertex sets per object
#define RT_TILEMASK_SETS 64          // ... and per scene (12 KiB): later objects go without

// What the predicate reads of a scene (host: tilemask_scene in k_masks.hip; the device copy lives in
// the scene blob).
struct RtTileMaskScene {
  RtCamera cam;
  int32_t width, height;
  int32_t n_objects;                 // <= RT_TILEMASK_OBJECTS, else `valid` is 0
  int32_t n_lights;
  int32_t plane;                     // the mask plane's object index, -1: none
  int32_t refl_ok;                   // the plane's shading normal is its geometric one (see above)
  int32_t valid;                     // 0: every word of every tile is all ones
  uint32_t boxed;                    // bit o: object o has a finite box (cull == RT_CULL_BOX)
  double pn[3], pd;                  // the mask plane in world space: pn . x + pd = 0
  double blo[RT_TILEMASK_OBJECTS][3], bhi[RT_TILEMASK_OBJECTS][3];
  double light[RT_TILEMASK_LIGHTS][3];
  // Tighter bounds of a boxed object's accepted hits (see "vertex sets" above): object o's sets are
  // sets[set_begin[o] .. set_begin[o + 1]), at most RT_TILEMASK_OBJ_SETS each; ball[o] = centre and
  // squared radius where bit o of `balled` is set.
  uint32_t balled;
  int32_t set_begin[RT_TILEMASK_OBJECTS + 1];
  double ball[RT_TILEMASK_OBJECTS][4];
  double sets[RT_TILEMASK_SETS][8][3];   // corner k's neighbours along the box's edges are k^1, k^2, k^4
};

struct TmV { double x, y, z; };
RT_TM_HD TmV tm_sub(TmV a, TmV b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_TM_HD double tm_dot(TmV a, TmV b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RT_TM_HD TmV tm_cross(TmV a, TmV b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RT_TM_HD TmV tm_ld(const double* p) { return {p[0], p[1], p[2]}; }
RT_TM_HD bool tm_in_range(TmV a) {
  return fabs(a.x) <= RT_CULL_COORD_MAX && fabs(a.y) <= RT_CULL_COORD_MAX && fabs(a.z) <= RT_CULL_COORD_MAX;
}

// Are the box's 8 corners all strictly outside the half-space n . (x - apex) >= 0?  The tolerance is
// 1e-12 of the dot product's magnitude; NaN answers no.
RT_TM_HD bool tm_all_outside(TmV n, TmV apex, const double* lo, const double* hi) {
  for (int k = 0; k < 8; ++k) {
    const TmV c = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
    const double s = tm_dot(n, tm_sub(c, apex));
    const double mag = fabs(n.x) * (fabs(c.x) + fabs(apex.x)) + fabs(n.y) * (fabs(c.y) + fabs(apex.y)) +
                       fabs(n.z) * (fabs(c.z) + fabs(apex.z));
    if (!(s < -1e-12 * mag)) return false;
  }
  return true;
}

// The signed value n . (c - apex) of a point and the magnitude its tolerance is taken of; `a` bounds |c|
// per coordinate (|c| itself for a corner, the larger endpoint for a point on an edge).
RT_TM_HD bool tm_pt_outside(TmV n, TmV apex, TmV c, TmV a, double tol) {
  const double s = tm_dot(n, tm_sub(c, apex));
  const double mag = fabs(n.x) * (a.x + fabs(apex.x)) + fabs(n.y) * (a.y + fabs(apex.y)) + fabs(n.z) * (a.z + fabs(apex.z));
  return s < -tol * mag;
}
RT_TM_HD TmV tm_abs(TmV c) { return {fabs(c.x), fabs(c.y), fabs(c.z)}; }
RT_TM_HD void tm_box_corners(const double* lo, const double* hi, TmV c[8]) {
  for (int k = 0; k < 8; ++k) c[k] = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
}

// tm_all_outside for the part of the box-shaped vertex set c[0..7] (corner k's edge neighbours are
// k^1, k^2, k^4) inside the half-space cn . (x - cp) >= 0: a convex polytope whose vertices are the
// corners inside and the points where an edge crosses the clipping plane, so a linear function that is
// negative on all of those is negative on all of it.  A corner counts as inside unless it is outside by
// the corner tolerance (NaN: inside), so the clipped part only grows.  A crossing point is
// c[k] + t (c[j] - c[k]), t = s_k / (s_k - s_j) clamped to [0, 1]: the two signed values carry rounding
// of <= 1e-15 of `magc`, so where s_k - s_j >= 1e-6 magc the point is off along the edge by < 4e-9 of
// its length, < 8e-9 of the side test's magnitude, and is tested with 1e-7; an edge flatter to the
// clipping plane than that is kept whole (its outside corner is tested too).  Nothing inside: outside.
RT_TM_HD bool tm_clip_outside(const TmV c[8], TmV n, TmV apex, TmV cn, TmV cp) {
  double s[8];
  bool in[8];
  for (int k = 0; k < 8; ++k) {
    s[k] = tm_dot(cn, tm_sub(c[k], cp));
    const double mag = fabs(cn.x) * (fabs(c[k].x) + fabs(cp.x)) + fabs(cn.y) * (fabs(c[k].y) + fabs(cp.y)) +
                       fabs(cn.z) * (fabs(c[k].z) + fabs(cp.z));
    in[k] = !(s[k] < -1e-12 * mag);
  }
  for (int k = 0; k < 8; ++k) {
    if (!in[k]) continue;
    if (!tm_pt_outside(n, apex, c[k], tm_abs(c[k]), 1e-12)) return false;
    for (int b = 1; b < 8; b <<= 1) {
      const int j = k ^ b;
      if (in[j]) continue;
      const TmV a = {fmax(fabs(c[k].x), fabs(c[j].x)), fmax(fabs(c[k].y), fabs(c[j].y)), fmax(fabs(c[k].z), fabs(c[j].z))};
      const double magc = fabs(cn.x) * (a.x + fabs(cp.x)) + fabs(cn.y) * (a.y + fabs(cp.y)) + fabs(cn.z) * (a.z + fabs(cp.z));
      const double den = s[k] - s[j];
      if (!(den >= 1e-6 * magc)) {                         // nearly in the clipping plane (or NaN): the whole edge
        if (!tm_pt_outside(n, apex, c[j], tm_abs(c[j]), 1e-12)) return false;
        continue;
      }
      double t = s[k] / den;
      t = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;             // NaN: 0, the corner itself
      const TmV p = {c[k].x + (c[j].x - c[k].x) * t, c[k].y + (c[j].y - c[k].y) * t, c[k].z + (c[j].z - c[k].z) * t};
      if (!tm_pt_outside(n, apex, p, a, 1e-7)) return false;
    }
  }
  return true;
}

// The ball (centre b[0..2], squared radius b[3]) lies strictly outside the half-space n . (x - apex) >= 0:
// the centre's signed distance is below -radius, compared as squares (no square root: the same bits on
// host and device) with 1e-9 to spare; NaN answers no.
RT_TM_HD bool tm_ball_outside(TmV n, TmV apex, const double* b) {
  const TmV c = {b[0], b[1], b[2]};
  const double s = tm_dot(n, tm_sub(c, apex));
  return tm_pt_outside(n, apex, c, tm_abs(c), 1e-12) && s * s > b[3] * tm_dot(n, n) * (1.0 + 1e-9);
}

// The same for the part of the ball inside the half-space cn . (x - cp) >= 0.  With h = cn . (c - cp) and
// g = cn . n: the part is empty when h < -r |cn|.  Otherwise n . (x - apex) is largest over the whole ball at
// c + r n / |n|; where that point lies beyond the clipping plane (h + r g / |n| < 0) the largest value over
// the part is taken on the disc the plane cuts out of the ball -- centre c' = c - (h / cn.cn) cn, squared
// radius r^2 - h^2 / cn.cn -- and is n . (c' - apex) + radius |n_t|, n_t = n less its component along cn.
// Everything is compared as squares, each with 1e-9 to spare on the side that keeps; where the highest
// point is not clearly beyond the plane only the whole ball is asked (the two bounds meet there).
RT_TM_HD bool tm_ball_outside_clipped(TmV n, TmV apex, const double* b, TmV cn, TmV cp) {
  if (tm_ball_outside(n, apex, b)) return true;
  const TmV c = {b[0], b[1], b[2]};
  const double N2 = tm_dot(cn, cn), n2 = tm_dot(n, n), h = tm_dot(cn, tm_sub(c, cp)), g = tm_dot(cn, n);
  if (!(N2 > 0.0 && n2 > 0.0 && b[3] >= 0.0)) return false;
  const double magh = fabs(cn.x) * (fabs(c.x) + fabs(cp.x)) + fabs(cn.y) * (fabs(c.y) + fabs(cp.y)) + fabs(cn.z) * (fabs(c.z) + fabs(cp.z));
  const bool below = h < -1e-12 * magh;
  if (below && h * h > b[3] * N2 * (1.0 + 1e-9)) return true;          // nothing of the ball inside
  const bool beyond = g >= 0.0 ? below && h * h * n2 > b[3] * g * g * (1.0 + 1e-9)
                               : below || h * h * n2 * (1.0 + 1e-9) < b[3] * g * g;
  if (!beyond) return false;
  const double k = h / N2;
  const TmV d = {cn.x * k, cn.y * k, cn.z * k}, cd = tm_sub(c, d);
  const TmV a = {fabs(c.x) + fabs(d.x), fabs(c.y) + fabs(d.y), fabs(c.z) + fabs(d.z)};
  double rho2 = b[3] - h * k, nt2 = n2 - g * (g / N2);
  rho2 = (rho2 > 0.0 ? rho2 : 0.0) * (1.0 + 1e-9) + 1e-9 * b[3];
  nt2 = (nt2 > 0.0 ? nt2 : 0.0) + 1e-9 * n2;
  const double fc = tm_dot(n, tm_sub(cd, apex));
  return tm_pt_outside(n, apex, cd, a, 1e-9) && fc * fc > rho2 * nt2;
}

// Is object o outside the half-space n . (x - apex) >= 0: its box, else one of its vertex sets, else its ball.
RT_TM_HD bool tm_obj_outside(const RtTileMaskScene& S, int o, TmV n, TmV apex) {
  if (tm_all_outside(n, apex, S.blo[o], S.bhi[o])) return true;
  for (int q = S.set_begin[o]; q < S.set_begin[o + 1]; ++q) {
    bool out = true;
    for (int k = 0; k < 8 && out; ++k) {
      const TmV c = tm_ld(S.sets[q][k]);
      out = tm_pt_outside(n, apex, c, tm_abs(c), 1e-12);
    }
    if (out) return true;
  }
  return ((S.balled >> o) & 1u) && tm_ball_outside(n, apex, S.ball[o]);
}

// The same for the part of the object inside the half-space cn . (x - cp) >= 0.
RT_TM_HD bool tm_obj_outside_clipped(const RtTileMaskScene& S, int o, TmV n, TmV apex, TmV cn, TmV cp) {
  TmV c[8];
  tm_box_corners(S.blo[o], S.bhi[o], c);
  if (tm_clip_outside(c, n, apex, cn, cp)) return true;
  for (int q = S.set_begin[o]; q < S.set_begin[o + 1]; ++q) {
    for (int k = 0; k < 8; ++k) c[k] = tm_ld(S.sets[q][k]);
    if (tm_clip_outside(c, n, apex, cn, cp)) return true;
  }
  return ((S.balled >> o) & 1u) && tm_ball_outside_clipped(n, apex, S.ball[o], cn, cp);
}

// The four side planes (inward normals) of the cone / pyramid from `apex` through the points
// apex + v[0..3] (in order around the rim).  False: the four are not in convex position.
RT_TM_HD bool tm_side_planes(const TmV v[4], TmV n[4]) {
  const TmV vc = {v[0].x + v[1].x + v[2].x + v[3].x, v[0].y + v[1].y + v[2].y + v[3].y, v[0].z + v[1].z + v[2].z + v[3].z};
  for (int i = 0; i < 4; ++i) {
    const TmV a = v[i], b = v[(i + 1) & 3];
    TmV m = tm_cross(a, b);
    const double s = tm_dot(m, vc);
    if (!(s > 0.0) && !(s < 0.0)) return false;          // zero or NaN
    if (s < 0.0) m = {-m.x, -m.y, -m.z};
    // the other two rim vectors strictly inside this plane, by more than any rounding
    const double len2 = tm_dot(m, m);
    for (int j = 2; j < 4; ++j) {
      const TmV w = v[(i + j) & 3];
      const double t = tm_dot(m, w);
      if (!(t > 0.0 && t * t > 1e-18 * len2 * tm_dot(w, w))) return false;
    }
    n[i] = m;
  }
  return true;
}

// Clears from *word the boxed objects that lie outside one of the four side planes.
RT_TM_HD void tm_cull_sides(const RtTileMaskScene& S, const TmV n[4], TmV apex, uint32_t* word) {
  for (int o = 0; o < S.n_objects; ++o) {
    if (!((S.boxed >> o) & 1u) || !((*word >> o) & 1u)) continue;
    for (int i = 0; i < 4; ++i)
      if (tm_obj_outside(S, o, n[i], apex)) { *word &= ~(1u << o); break; }
  }
}

// The words of one tile whose valid pixels span [x0, x1] x [y0, y1] (frame coordinates, inclusive).
RT_TM_HD void tilemask_eval(const RtTileMaskScene& S, int x0, int x1, int y0, int y1, uint32_t out[RT_TILEMASK_WORDS]) {
  for (int k = 0; k < RT_TILEMASK_WORDS; ++k) out[k] = 0xffffffffu;
  if (!S.valid || x1 < x0 || y1 < y0) return;
  const RtCamera& cam = S.cam;
  const TmV C = tm_ld(cam.center);
  if (!tm_in_range(C)) return;
  // the grown rectangle's corner directions, camera_ray's expressions at fractional pixels
  const double xs[2] = {(double)x0 - 0.5, (double)x1 + 0.5}, ys[2] = {(double)y0 - 0.5, (double)y1 + 0.5};
  TmV d[4];
  for (int k = 0; k < 4; ++k) {
    const double x = xs[(k == 1 || k == 2) ? 1 : 0], y = ys[k >= 2 ? 1 : 0];
    const double sx = ((x / cam.width) - 0.5) * cam.aspect;
    const double sy = (cam.height - 1.0 - y) / cam.height - 0.5;
    d[k] = {cam.direction[0] + cam.right[0] * sx + cam.up[0] * sy, cam.direction[1] + cam.right[1] * sx + cam.up[1] * sy,
            cam.direction[2] + cam.right[2] * sx + cam.up[2] * sy};
    const double ad = fmax(fmax(fabs(d[k].x), fabs(d[k].y)), fabs(d[k].z));
    if (!(ad >= 1e-6 && ad <= 1e6)) return;               // NaN, zero or huge direction: all ones
  }
  TmV n[4];
  if (!tm_side_planes(d, n)) return;
  // ---- prim (a computed word holds no bit beyond the scene's objects)
  const uint32_t live = S.n_objects >= 32 ? 0xffffffffu : (1u << S.n_objects) - 1u;
  out[0] = live;
  tm_cull_sides(S, n, C, &out[0]);
  // ---- the mask plane
  if (S.plane < 0) return;
  const TmV pn = tm_ld(S.pn);
  const double pn2 = tm_dot(pn, pn), sC = tm_dot(pn, C) + S.pd;
  if (!(pn2 > 0.0 && pn2 <= 1e300) || !(sC > 0.0 || sC < 0.0)) return;
  // The plane itself (unbounded: its node ignores the mask, the bit only describes the tile): a ray meets
  // it at t = -sC / (pn . d) > 0 only where pn . d and sC have opposite signs; pn . d is linear in the
  // direction, so four corner rays that all clearly lead away from the plane bound every ray of the tile.
  bool away = true;
  for (int k = 0; k < 4; ++k) {
    const double vd = tm_dot(pn, d[k]);
    away = away && vd * sC > 0.0 && vd * vd >= 1e-8 * pn2 * tm_dot(d[k], d[k]);
  }
  if (away) out[0] &= ~(1u << S.plane);
  TmV Q[4];
  for (int k = 0; k < 4; ++k) {
    const double vd = tm_dot(pn, d[k]);
    if (!(vd * vd >= 1e-8 * pn2 * tm_dot(d[k], d[k]))) return;       // grazing, parallel or NaN
    const double t = -sC / vd;
    if (!(t > 0.0 && t <= 1e300)) return;                            // the corner ray leaves the plane
    Q[k] = {C.x + d[k].x * t, C.y + d[k].y * t, C.z + d[k].z * t};
    if (!tm_in_range(Q[k])) return;
  }
  // ---- shadow[l]
  if (S.n_lights <= RT_TILEMASK_LIGHTS) {
    for (int l = 0; l < S.n_lights; ++l) {
      const TmV L = tm_ld(S.light[l]);
      const double sL = tm_dot(pn, L) + S.pd;
      if (!tm_in_range(L) || !(sL * sL >= 1e-12 * pn2)) continue;    // light on the plane (or NaN): all ones
      uint32_t w = live;
      TmV v[4], m[4];
      for (int k = 0; k < 4; ++k) v[k] = tm_sub(Q[k], L);
      const bool sides = tm_side_planes(v, m);
      double alo[3] = {L.x, L.y, L.z}, ahi[3] = {L.x, L.y, L.z};
      for (int k = 0; k < 4; ++k) {
        alo[0] = fmin(alo[0], Q[k].x); ahi[0] = fmax(ahi[0], Q[k].x);
        alo[1] = fmin(alo[1], Q[k].y); ahi[1] = fmax(ahi[1], Q[k].y);
        alo[2] = fmin(alo[2], Q[k].z); ahi[2] = fmax(ahi[2], Q[k].z);
      }
      // inward normals of the two planes parallel to the mask plane: towards L at Q, towards Q at L
      const TmV up = sL > 0.0 ? pn : TmV{-pn.x, -pn.y, -pn.z}, down = {-up.x, -up.y, -up.z};
      for (int o = 0; o < S.n_objects; ++o) {
        if (!((S.boxed >> o) & 1u)) continue;
        const double* lo = S.blo[o];
        const double* hi = S.bhi[o];
        bool cull = tm_obj_outside(S, o, up, Q[0]) || tm_obj_outside(S, o, down, L);
        for (int a = 0; a < 3 && !cull; ++a) {
          const double tol = 1e-9 * (1.0 + fabs(alo[a]) + fabs(ahi[a]));
          cull = lo[a] > ahi[a] + tol || hi[a] < alo[a] - tol;
        }
        // the side planes see only what lies on the floor's side of the plane through L
        for (int i = 0; i < 4 && !cull && sides; ++i) cull = tm_obj_outside_clipped(S, o, m[i], L, down, L);
        if (cull) w &= ~(1u << o);
      }
      out[1 + l] = w;
    }
  }
  // ---- refl
  if (S.refl_ok) {
    const double k2 = 2.0 * sC / pn2;
    const TmV Cm = {C.x - pn.x * k2, C.y - pn.y * k2, C.z - pn.z * k2};     // the camera mirrored in the plane
    if (tm_in_range(Cm)) {
      TmV v[4], m[4];
      for (int k = 0; k < 4; ++k) v[k] = tm_sub(Q[k], Cm);
      uint32_t w = live;
      if (tm_side_planes(v, m)) tm_cull_sides(S, m, Cm, &w);
      const TmV cs = sC > 0.0 ? pn : TmV{-pn.x, -pn.y, -pn.z};              // towards the camera's side
      for (int o = 0; o < S.n_objects; ++o)
        if (((S.boxed >> o) & 1u) && ((w >> o) & 1u) && tm_obj_outside(S, o, cs, Q[0])) w &= ~(1u << o);
      out[5] = w;
    }
  }
}

// The valid pixels of tile `tile` of a band launch (rt_device.h tile_pixel and band_row, restated for
// the host): their frame rectangle.  False: the tile has no valid pixel.
RT_TM_HD bool tilemask_rect(unsigned tile, int width, int height, int y_first, int band_rows, int band_pitch, int n_rows,
                            int* x0, int* x1, int* y0, int* y1) {
  const int tile_h = 64 / RT_TILE_W;
  const unsigned tiles_x = (unsigned)(width + RT_TILE_W - 1) / RT_TILE_W;
  const int xa = (int)(tile % tiles_x) * RT_TILE_W, ra = (int)(tile / tiles_x) * tile_h;
  *x0 = xa;
  *x1 = xa + RT_TILE_W - 1 < width - 1 ? xa + RT_TILE_W - 1 : width - 1;
  bool any = false;
  for (int r = ra; r < ra + tile_h && r < n_rows; ++r) {
    const int y = band_rows >= n_rows ? y_first + r : y_first + (r / band_rows) * band_pitch + r % band_rows;
    if (y >= height) continue;
    if (!any) { *y0 = y; *y1 = y; any = true; }
    if (y < *y0) *y0 = y;
    if (y > *y1) *y1 = y;
  }
  return any && *x0 <= *x1;
}
