// rt_trace.h -- the third part of the device core (rt_device.h; after rt_walks.h): a hit's normal, UV and
// texture colour, the inside test, reflection and refraction directions, the wave-scalarised shading
// inputs, the ray-debugger recorders, the frame stack's LDS slots and the wave pool, and get_ray_color
// itself as trace() (one ray tree per lane) and trace_deferred() (chain, wave-wide shadows, fold).
#pragma once

namespace {

// Normal and UV of top-level object O at point p: RTObject shape get_normal / get_uv_coordinates,
// with CSG's is_on_surface / is_inside evaluated bottom-up over the post-order node list
// (csg.rs:98-168) and the descent a-then-b of csg.rs:104-121 / :161-167.
RT_FN void object_normal_uv(const DS& S, cptr<RtObject> O, V3 p, bool want_uv, V3* n,
                                 double* u, double* v) {
  cptr<RtNode> N = S.nodes + O->node_begin;
  const int cnt = O->node_count;
  const bool fin = wave_finite(p);
  *u = 0.0;
  *v = 0.0;
  // want_uv: the object is textured; its texture's size arms sphere_uv's texel-boundary guard
  const int tw = want_uv ? S.textures[O->tex].w : 0, th = want_uv ? S.textures[O->tex].h : 0;
  if (cnt == 1) {
    RT_REC(L, S, leaves, LEAVES, N[0].leaf);
    *n = leaf_normal(L, p, fin);
    if (want_uv && L->kind == RT_N_SPHERE) sphere_uv(L, p, u, v, tw, th);
    return;
  }
  uint32_t in = 0, on = 0;
  RT_SPEC_UNROLL
  for (int i = 0; i < cnt; ++i) {
    const int nk = N[i].kind, na = N[i].a, nb = N[i].b, nl = N[i].leaf;
    bool bi, bo;
    if (nk < RT_N_UNION) {
      RT_REC(L, S, leaves, LEAVES, nl);
      bi = leaf_inside(L, p, fin);
      bo = leaf_on_surface(L, p, fin);
    } else {
      bool ia = (in >> na) & 1u, ib = (in >> nb) & 1u, oa = (on >> na) & 1u, ob = (on >> nb) & 1u;
      if (nk == RT_N_UNION) { bi = ia || ib; bo = (oa && !ib) || (ob && !ia); }
      else if (nk == RT_N_INTERSECTION) { bi = ia && ib; bo = (oa && ib) || (ob && ia); }
      else { bi = ia && !ib; bo = (oa && !ib) || (ob && ia); }
    }
    in |= (uint32_t)bi << i;
    on |= (uint32_t)bo << i;
  }
  // Descent a-then-b (csg.rs:104-121, :161-167).  Children precede parents in post-order, so one
  // downward pass over the node indices visits every lane's path in order; node reads stay
  // wave-uniform (scalar).  Membership tests go through ballot masks (see trace()).
  const int lane = __lane_id();
  int cur = cnt - 1, sel = -1;
  bool neg = false;
  RT_SPEC_UNROLL
  for (int i = cnt - 1; i >= 0; --i) {
    const int nk = N[i].kind, na = N[i].a, nb = N[i].b, nl = N[i].leaf;
    if (!((__ballot(cur == i) >> lane) & 1)) continue;
    if (nk < RT_N_UNION) { sel = nl; cur = -1; }
    else if ((on >> na) & 1u) cur = na;
    else if ((on >> nb) & 1u) { if (nk == RT_N_DIFFERENCE) neg = !neg; cur = nb; }   // b.get_normal(p) * -1.0
    else cur = -1;                                          // fallback (1,0,0); UV is Err -> (0,0)
  }
  *n = {1.0, 0.0, 0.0};
  const int lb = O->leaf_begin, le = lb + O->leaf_count;
  RT_SPEC_UNROLL
  for (int l = lb; l < le; ++l) {
    if (!((__ballot(sel == l) >> lane) & 1)) continue;
    RT_REC(L, S, leaves, LEAVES, l);
    *n = leaf_normal(L, p, fin);
    if (want_uv && L->kind == RT_N_SPHERE) sphere_uv(L, p, u, v, tw, th);
  }
  if (neg) *n = scale(*n, -1.0);
}

// PixmapTexture::get_color_at (texture.rs:27-34) on RGBA8 texels, /255.0 (sceneparser/texture.rs:29-33)
RT_FN Col texture_color(const DS& S, int tex, double u, double v) {
  const int tw = S.textures[tex].w, th = S.textures[tex].h;
  const int64_t toff = S.textures[tex].offset;
  double x = u * (double)(tw - 1);
  double y = (double)th - (v * (double)(th - 1)) - 1.0;
  // `as usize` saturates (NaN/negative -> 0); the reference would panic past the edge: clamp.
  int xi = x > 0.0 ? (x < (double)(tw - 1) ? (int)x : tw - 1) : 0;
  int yi = y > 0.0 ? (y < (double)(th - 1) ? (int)y : th - 1) : 0;
  const uint32_t px = *(const uint32_t*)(S.texels + toff + ((size_t)yi * tw + xi) * 4);
  return {(double)(px & 0xffu) / 255.0, (double)((px >> 8) & 0xffu) / 255.0, (double)((px >> 16) & 0xffu) / 255.0};
}

// angle(-dir, n) >= PI/2 (raytracer.rs:230-231) from the cosine `cin` the angle's acos would take
// (vector.rs:57-59).  acos is monotone and rt_acos is within 1 ulp, so for |cin| > 1e-15 (>= 4 ulp
// of PI/2 away from the threshold) the sign decides exactly -- except past -1: a cosine that
// rounds below -1 (a ray through a sphere's centre meets the normal head-on) makes acos NaN and
// the comparison false, so such a hit is NOT inside.  Near-grazing cosines (and NaN) evaluate
// the acos itself.
__device__ __forceinline__ bool inside_test(double cin) {
  return cin < -1e-15 ? cin >= -1.0 : (cin > 1e-15 ? false : rt_acos(cin) >= PI_D / 2.0);
}
// inside_test's "outside" answer without the square root and the division, for cin = d / (len(a) * nl)
// with q = dot(a, a) (len(a) = sqrt(q)): when d > 0 and d^2 > 1e-30 q nl^2 (1 + 2^-40), with the right
// side a normal double, the computed cin exceeds 1e-15 -- sqrt, product and quotient round by 2^-53
// each, the squares and products here by as much, and 2^-40 covers them all -- so inside_test answers
// false.  Anything else (NaN, overflow, grazing, inside) takes the exact path.  A wave of hits seen
// from outside (floor pixels, every primary hit) skips len() and the division.
__device__ __forceinline__ bool outside_certain(double d, double q, double nl) {
  const double rhs = (1e-30 * q) * (nl * nl) * (1.0 + 0x1p-40);
  return d > 0.0 && rhs >= 0x1p-1000 && d * d > rhs;
}

// ang / (PI / 2) of the Lambert term (raytracer.rs:216-218) for ang in [0, PI/2): an acos result there is
// +0 or at least acos(1 - 2^-53) > 1e-8 (never subnormal), so div_core's conditions hold (no scaling in
// either v_div_scale; a zero numerator keeps its sign through v_div_fixup): the compiler's division
// minus its identities, bit-identical.
__device__ __forceinline__ double lambert_ratio(double ang) {
  return div_core(ang, PI_D / 2.0);
}

__device__ __forceinline__ V3 reflect_dir(V3 i, V3 n) {                    // raytracer.rs:332-334
  return sub(i, scale(scale(n, 2.0), dot(n, i)));
}
__device__ __forceinline__ V3 refract_dir(V3 i, V3 n, double r, bool* tir) {   // raytracer.rs:336-353
  double cos_1 = dot(scale(i, -1.0), n);
  double v = 1.0 - r * r * (1.0 - cos_1 * cos_1);
  *tir = v < 0.0;
  if (*tir) return {0.0, 0.0, 0.0};
  double cos_2 = sqrt_rt(v);
  return normalized(add(scale(i, r), scale(n, r * cos_1 - cos_2)));
}

// Normal (normalised, :163), material colour at the UV (:165-170), transparency, reflectivity of
// each lane's hit object -- SCALARISED over the distinct objects hit in this wave (readlane of the
// first remaining lane), so every object / node / leaf read is wave-uniform (SMEM, no VGPRs).
// nlen (optional): len(normal) of the normalised normal, the denominator term the Lambert angles and the
// inside test take (vector.rs:57-59) -- formed once here.  Objects whose normal is a constant (a plane:
// RtObject::unit_normal) take the host's normalised normal and its length (the same IEEE operations on the
// same values: bit-identical), so a wave of floor hits skips the normalisation and the length.
__device__ __forceinline__ void shade_inputs(const DS& S, int oi, V3 p, V3* nrm, Col* c, double* transp,
                                             double* refl, double* nlen = nullptr) {
  RT_OPAQUE(p.x);                          // RT_SPEC: keep the per-object work on p in the light loop
  RT_OPAQUE(p.y);                          // (see RT_OPAQUE)
  RT_OPAQUE(p.z);
  bool unit = false;
  auto shade = [&](cptr<RtObject> O) RT_INL {
    double u = 0.0, v = 0.0;                 // a plane's UV is Err -> (0, 0) (math_shapes.rs:196-198)
    if (nlen && O->unit_normal) {
      *nrm = ld3(O->nunit);
      *nlen = O->nunit_len;
      unit = true;
    } else {
      object_normal_uv(S, O, p, O->textured != 0, nrm, &u, &v);
    }
    *c = O->textured ? texture_color(S, O->tex, u, v) : Col{O->color[0], O->color[1], O->color[2]};
    *transp = O->transparency;
    *refl = O->reflectivity;
  };
#ifdef RT_SPEC
  // every object's inputs are constants: one branch per object, taken by the lanes that hit it
  spec_for<0, rt_spec::N_OBJECTS>([&](auto I) RT_INL {
    constexpr int o = decltype(I)::value;
    if (oi == o) {
      RT_REC(O, S, objects, OBJECTS, o);
      shade(O);
    }
  });
#else
  uint64_t todo = __ballot(oi >= 0);
  while (todo) {
    const int o = __builtin_amdgcn_readlane(oi, (int)__builtin_ctzll(todo));
    const uint64_t mine = __ballot(oi == o);
    todo &= ~mine;
    // test membership through the ballot mask, not `oi == o`: an equality lets the optimiser
    // substitute the per-lane oi for the uniform o and the loads below turn into VMEM again.
    if ((mine >> __lane_id()) & 1) shade(&S.objects[o]);
  }
#endif
  if (!unit) {
    *nrm = normalized(*nrm);
    if (nlen) *nlen = len(*nrm);
  }
}

template <class A, class B> struct same_type { static constexpr bool value = false; };
template <class A> struct same_type<A, A> { static constexpr bool value = true; };


// Ray-debugger recording (raytracer.rs:17-19, :155-157, :282-284; ray_debugger.rs:92-137).
// NoRec compiles to nothing in the render kernels; RtRayRecord slots are written in ray START
// order and `order` lists them in the reference's callback order (a ray reports after its
// children: post-order).
struct NoRec {
  __device__ __forceinline__ int begin(int, int, V3, V3, double, int, V3) { return 0; }
  __device__ __forceinline__ void finish(int, Col) {}
};
#ifndef __HIPCC_RTC__
using RtRayRecord = rt_ray_record;
struct BufRec {
  RtRayRecord* rec;
  int* order;
  int cap, n_begun, n_done;
  const DS* S;
  __device__ int begin(int depth, int type, V3 ro, V3 rd, double t, int oi, V3 p) {
    const int i = n_begun++;
    if (i >= cap) return -1;
    RtRayRecord& r = rec[i];
    r.depth = depth; r.ray_type = type; r.object = oi; r.intersected = t != INFINITY;
    r.point[0] = ro.x; r.point[1] = ro.y; r.point[2] = ro.z;
    r.direction[0] = rd.x; r.direction[1] = rd.y; r.direction[2] = rd.z;
    r.distance = t;
    const V3 ip = add(ro, scale(rd, r.intersected ? t : 1000.0));          // ray_debugger.rs:107-111
    r.intersection[0] = ip.x; r.intersection[1] = ip.y; r.intersection[2] = ip.z;
    r.has_normal = oi >= 0;
    V3 n = {0.0, 0.0, 0.0};
    if (oi >= 0) {                                                         // shape.get_normal (:113-119)
      double u, v;
      object_normal_uv(*S, &S->objects[oi], ip, false, &n, &u, &v);
    }
    r.normal[0] = n.x; r.normal[1] = n.y; r.normal[2] = n.z;
    return i;
  }
  __device__ void finish(int i, Col c) {
    if (i < 0) return;
    rec[i].color[0] = c.r; rec[i].color[1] = c.g; rec[i].color[2] = c.b; rec[i].color[3] = 1.0;
    if (n_done < cap) order[n_done] = i;
    ++n_done;
  }
};
#endif

// Frame-stack slots in LDS.  The first KL frames of every lane's stack (A.r, A.g, A.b, w) live in
// LDS laid out [frame][component][lane], so each access is one conflict-free ds_*_b64; deeper
// frames (chains longer than KL, rare) use the private array, i.e. scratch.  Refraction frames of the
// ray-tree mode also carry the pending reflection ray (P, D, rp: 7 doubles); the first KLR of them go
// to LDS after the KL colour frames, [frame][component][lane] likewise.  (KL, KLR and the pool's KP per
// kernel mode: rt_tunables.h, rows_lane_frames / rows_pool_slots in rt_bodies.h.)
#define LDS_AS __attribute__((address_space(3)))
typedef LDS_AS double lds_f64;

// The wave's frame POOL (KP > 0, chain and reflection-only kernels, round 5): instead of KL frames per
// lane, the wave's LDS holds KP frame slots shared by its 64 lanes.  In those modes every hit spawns at
// most one ray, so the lanes still walking push their frame f in the same iteration f: one ballot gives
// the pushing lanes m, each takes slot start + (its rank in m) (mbcnt), and (m, start) are kept per f
// (pool_mask / pool_start) so that a lane folding its frame f later finds its slot again.  Lanes whose
// chains are short leave their share to the long ones: a spinning_globes wave needs ~2 frames per lane
// on average but up to 10 for some lanes, so the fixed per-lane layout either spilled the deep frames
// to scratch (KL = 5: 48.7 MB of HBM per 1080p frame) or cost occupancy.  Slots past KP, and frames of
// pixels whose chain outgrows the pool, use the private array (scratch).  The first KL frames of every
// lane keep their fixed per-lane LDS slots (most chains are that short, and a fixed slot costs no
// ballot, no rank and no header reads); the pool serves the deeper ones.  Layout at the wave's base lp:
// [KL][4][64] per-lane frames, [RT_MAX_DEPTH_CAP] u64 masks, [RT_MAX_DEPTH_CAP] u32 starts, then [4][KP]
// doubles (component-major: the lanes of one push write consecutive doubles).
constexpr int RT_POOL_HDR = RT_MAX_DEPTH_CAP + RT_MAX_DEPTH_CAP / 2;      // header doubles
#define LDS_U64 __attribute__((address_space(3))) uint64_t
#define LDS_U32 __attribute__((address_space(3))) uint32_t
#define LDS_U8 __attribute__((address_space(3))) uint8_t
// Pool slots hold (A, hit object) instead of (A, w) (round 6).  Outside the ray-tree mode a frame's
// weight is a function of the hit object alone: a refraction frame's w is the object's transparency; a
// reflection frame's is rp = TIR ? refl + (1 - refl) * transp : refl (raytracer.rs:261-265), and a TIR
// hit refracts only where transp != 0, which in these modes forces refl == +-0, so rp = 0 + 1 * transp
// = transp exactly; without TIR a reflecting object has transp == 0 (else it would have refracted), so
// w = refl.  Hence w = (transp != 0 ? transp : refl) of the frame's object (frame_weight), bit for bit,
// and a slot is 3 doubles + 1 byte: 25 B instead of 32.  Scenes of more than 256 objects keep w.
#ifndef RT_POOL_OBJ_INDEX
#define RT_POOL_OBJ_INDEX 1
#endif
template <int KP, bool PIDX> constexpr int pool_doubles() { return PIDX ? 3 * KP + (KP + 7) / 8 : 4 * KP; }
// the weight of a frame whose hit object is o (see RT_POOL_OBJ_INDEX)
__device__ __forceinline__ double frame_weight(const DS& S, int o) {
#ifdef RT_SPEC
  double w = 0.0;
  spec_for<0, rt_spec::N_OBJECTS>([&](auto I) RT_INL {
    constexpr int k = decltype(I)::value;
    RT_REC(O, S, objects, OBJECTS, k);
    const double t = O->transparency;
    if (o == k) w = t != 0.0 ? t : O->reflectivity;
  });
  return w;
#else
  const double t = S.objects[o].transparency;          // per-lane loads (the generic kernels)
  return t != 0.0 ? t : S.objects[o].reflectivity;
#endif
}
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {                 // set lanes of m below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// A wave's tile-mask words (rt_tilemask.h) as trace() takes them: wave-uniform values the caller read with
// the wave's dispatch record (rows_entry), scalar registers for the whole trace; all ones without a table.
// hit_min: the record's flag (RtTileRec r0's sign bit: words 1..5 hold for every depth-0 hit of the wave) as the
// scalar trace()'s depth-0 ballot compares hit objects with -- 0, or INT32_MAX where the flag is set, so that no
// hit counts as off the plane.  (The flag as a boolean ORed to the ballot's result cost the 4K globes megakernel
// two spilled VGPRs; as the ballot's own operand, none.)
struct TileMask { uint32_t w[RT_TILEMASK_WORDS]; int32_t hit_min; };
__device__ __forceinline__ TileMask tile_mask_ones() {
  TileMask m;
  for (int k = 0; k < RT_TILEMASK_WORDS; ++k) m.w[k] = 0xffffffffu;
  m.hit_min = 0;
  return m;
}

// The light of a hit (raytracer.rs:172-228) and its inside test (:230-235), each written ONCE, as statement
// macros: trace() expands them in place and the lean kernel's functions (hit_lights, hit_inside below) expand the
// same text, so the two cannot diverge.  They are macros and not functions that trace() calls because the same
// statements behind an inlined call cost the 4K globes megakernel two spilled VGPRs; expanded
// in place trace() compiles to the code it had.
// RT_HIT_LIGHTS: over the names S, oi, p (the hit), FC, SHARE, OBB, and nrm, c, L, transp, refl, nlen, which it
// sets.  SMASK: statements that may set `smask`, the tile-mask word of light k's shadow walk (all ones: none).
// Evaluation order is free (every step is a pure function of the hit), so the shadow
// rays of a group of lights are traced FIRST, while only the hit point is live, and the
// normal / UV / material and the per-light Lambert terms are formed afterwards: far fewer
// registers live across the traversals.  Light accumulation order is unchanged.
// One light at a time: the unit vector towards the light is the shadow ray's direction
// (:176-178) AND the Lambert term's `sdir` (:203-205), the same operations on the same
// operands, so it is formed once and kept for the Lambert term.
#define RT_HIT_LIGHTS(SMASK)                                                                         \
  {                                                                                                  \
    bool have_shading = false;                                                                       \
    _Pragma("unroll 1") for (int k = 0; k < S.n_lights; ++k) {                                       \
      RT_REC(lt, S, lights, LIGHTS, k);                                                              \
      const V3 lv = sub(ld3(lt->p), p);                                                              \
      double ll, ill;                                                                                \
      len_inv(lv, &ll, &ill);                                                                        \
      const V3 sdir = scale(lv, ill);                                    /* normalized(lv) */        \
      double t;                                                          /* :176-197 */              \
      uint32_t smask = 0xffffffffu;                                                                  \
      SMASK                                                                                          \
      t = shadow_transparency<SHARE, OBB>(S, p, sdir, ll, smask);                                    \
      if (!have_shading) {                                                                           \
        shade_inputs(S, oi, p, &nrm, &c, &transp, &refl, &nlen);                                     \
        L = cmul<FC>(c, in_range<FC>(0.6, 0.6, 0.6));                      /* ambient (:172) */      \
        have_shading = true;                                                                         \
      }                                                                                              \
      if (t == 0.0) continue;                                            /* :199-227 */              \
      double ang = rt_acos(dot(sdir, nrm) / (len(sdir) * nlen));                                     \
      if (ang >= PI_D / 2.0) ang = PI_D - ang;                                                       \
      const double inten = (ang < (PI_D / 2.0) && ang >= 0.0) ? 1.0 - lambert_ratio(ang) : 0.0;      \
      const Col lc = intensify<FC>(intensify<FC>(Col{lt->col[0], lt->col[1], lt->col[2]}, inten), t); \
      L = cadd<FC>(L, cmul<FC>(c, lc));                                                              \
    }                                                                                                \
    if (!have_shading) {                                                                             \
      shade_inputs(S, oi, p, &nrm, &c, &transp, &refl, &nlen);                                       \
      L = cmul<FC>(c, in_range<FC>(0.6, 0.6, 0.6));                                                  \
    }                                                                                                \
  }
// RT_HIT_INSIDE: sets `inside` from the ray direction rd and the hit's nrm, nlen.
#define RT_HIT_INSIDE()                                                                              \
  {                                                                                                  \
    const V3 nd = scale(rd, -1.0);                                                                   \
    const double d = dot(nd, nrm);                                                                   \
    if (!(outside_certain(d, dot(nd, nd), nlen)))                                                    \
      inside = inside_test(d / (len(nd) * nlen));                                                    \
  }
// The same as functions, for the lean kernel (rt_bodies.h lean_pixel): every shadow walk under the mask `smask_all`.
template <bool FC, bool SHARE, bool OBB>
RT_FN Col hit_lights(const DS& S, int oi, V3 p, uint32_t smask_all, V3* nrm_out, Col* c_out, double* transp_out,
                     double* refl_out, double* nlen_out) {
  V3 nrm = {0.0, 0.0, 0.0};
  Col c = {0.0, 0.0, 0.0}, L = {0.0, 0.0, 0.0};
  double transp = 0.0, refl = 0.0, nlen = 0.0;
  RT_HIT_LIGHTS(smask = smask_all;)
  *nrm_out = nrm; *c_out = c; *transp_out = transp; *refl_out = refl; *nlen_out = nlen;
  return L;
}
__device__ __forceinline__ bool hit_inside(V3 rd, V3 nrm, double nlen) {
  bool inside = false;
  RT_HIT_INSIDE()
  return inside;
}

// get_ray_color (raytracer.rs:132-287) for one primary ray, recursion unrolled onto a per-lane
// frame stack.  REFR = the scene has a transparent object (refraction frames need more state).
// KL > 0: frames 0..KL-1 of the stack are in LDS at lf[(f * 4 + c) * 64] (lf = this lane's slot);
// KLR > 0 (REFR): the pending-reflection state of frames 0..KLR-1 at lf[(KL * 4 + f * 7 + c) * 64].
// KP > 0 (not TREE, no recorder): frames KL.. go to the wave's pool of KP slots (above), after the KL
// per-lane frames at lp.
// CHAIN (REFR scenes with RtDevScene::ray_chains): every hit spawns at most one ray, so a refraction
// frame never carries a pending reflection: frames are (A, w) as in the reflection-only kernels.
template <bool REFR, class Rec = NoRec, int KL = 0, bool FC = false, int KLR = 0, bool CHAIN = false, int KP = 0>
RT_FN Col trace(const DS& S, V3 ro, V3 rd, int max_depth, Rec* rec = nullptr, lds_f64* lf = nullptr,
                lds_f64* lp = nullptr, const TileMask tm = tile_mask_ones()) {
  // Tile masks (rt_tilemask.h): the wave's RT_TILEMASK_WORDS words, scalars (all ones without a table; a
  // second form of this function that also kept the table's lazy scalar loads behind a wave-uniform branch
  // gave back 1.6 % of the 4K frame).  Reflection-only kernels: every hit spawns at most
  // one ray and a lane that spawns none leaves the loop, so iteration k traces the depth-k rays of the lanes still here.  The depth-0
  // nearest hit takes `prim`; where every lane that hit something hit the mask plane (one ballot, kept
  // in a scalar) or the wave's record says its words were traced for every hit (tm.hit_min, the ballot's own
  // operand), light l's depth-0 shadow walk takes shadow[l] and the depth-1 nearest hit `refl`;
  // every other walk takes all ones.  One walk either way: the mask is an operand, not a second copy.
#if defined(RT_SPEC) && RT_TILE_MASKS
  constexpr bool MASKS = !REFR && same_type<Rec, NoRec>::value;
  constexpr int mask_plane = rt_spec::MASK_PLANE;
#else
  constexpr bool MASKS = false;
  constexpr int mask_plane = -1;
#endif
  // depth 0: the wave's shadow[l] and refl words hold for its hits -- every hit is on the mask plane (what the
  // predicate's words are made for), or the record says its words were traced for every hit (tm.hit_min)
  [[maybe_unused]] bool plane_tile = false;
  double fA[RT_MAX_DEPTH_CAP][3];     // parent colour already intensified by (1 - w)
  double fW[RT_MAX_DEPTH_CAP];        // child weight w (transparency or reflectivity)
  constexpr bool POOL = KP > 0 && !(REFR && !CHAIN) && same_type<Rec, NoRec>::value;
  // pool slots hold the hit object instead of w (RT_POOL_OBJ_INDEX); the scene has <= 256 objects (host)
  constexpr bool PIDX = POOL && RT_POOL_OBJ_INDEX;
  // frames 0..KL-1 stay in the lanes' own LDS slots (lf); the pool serves frames KL.. (after them at lp)
  LDS_U64* const pool_mask = (LDS_U64*)(lp + KL * 4 * 64);
  LDS_U32* const pool_start = (LDS_U32*)(lp + KL * 4 * 64 + RT_MAX_DEPTH_CAP);
  lds_f64* const pool = lp + KL * 4 * 64 + RT_POOL_HDR;
  LDS_U8* const pool_obj = (LDS_U8*)(pool + 3 * KP);             // PIDX: [KP] object bytes after [3][KP] doubles
  uint32_t pool_used = 0;             // wave-uniform: slots taken by the pushes so far
  auto put_frame = [&](int f, Col A, double w) {
    if (KL > 0 && f < KL) {
      lf[(f * 4 + 0) * 64] = A.r; lf[(f * 4 + 1) * 64] = A.g; lf[(f * 4 + 2) * 64] = A.b; lf[(f * 4 + 3) * 64] = w;
    } else {
      fA[f][0] = A.r; fA[f][1] = A.g; fA[f][2] = A.b; fW[f] = w;
    }
  };
  auto get_frame = [&](int f, Col* A, double* w) {
    if (POOL && f >= KL) {
      const uint32_t slot = pool_start[f] + lane_rank(pool_mask[f]);
      if (slot < (uint32_t)KP) {
        *A = {pool[slot], pool[KP + slot], pool[2 * KP + slot]};
        if constexpr (PIDX) *w = frame_weight(S, pool_obj[slot]);
        else *w = pool[3 * KP + slot];
        return;
      }
    }
    if (KL > 0 && f < KL) {
      *A = {lf[(f * 4 + 0) * 64], lf[(f * 4 + 1) * 64], lf[(f * 4 + 2) * 64]}; *w = lf[(f * 4 + 3) * 64];
    } else {
      *A = {fA[f][0], fA[f][1], fA[f][2]}; *w = fW[f];
    }
  };
  // POOL: the frame every lane still walking pushes in this iteration (they are all at frame f)
  auto pool_push = [&](bool push, int f, Col A, double w, int obj) {
    const uint64_t m = __ballot(push);
    const uint32_t start = pool_used;
    if (push) {
      const uint32_t slot = start + lane_rank(m);
      if (slot < (uint32_t)KP) {
        pool[slot] = A.r; pool[KP + slot] = A.g; pool[2 * KP + slot] = A.b;
        if constexpr (PIDX) pool_obj[slot] = (uint8_t)obj;
        else pool[3 * KP + slot] = w;
      } else {
        fA[f][0] = A.r; fA[f][1] = A.g; fA[f][2] = A.b; fW[f] = w;
      }
      pool_mask[f] = m;                 // every pushing lane writes the same (m, start)
      pool_start[f] = start;
    }
    pool_used = start + (uint32_t)__builtin_popcountll(m);
  };
  constexpr bool TREE = REFR && !CHAIN;       // a hit may spawn two rays: pending reflections
  double fP[TREE ? RT_MAX_DEPTH_CAP : 1][3], fD[TREE ? RT_MAX_DEPTH_CAP : 1][3];
  double fRP[TREE ? RT_MAX_DEPTH_CAP : 1];
  uint32_t pend = 0;                  // bit f: frame f's reflection ray is still to be traced
  static_assert(RT_MAX_DEPTH_CAP <= 32, "pending-reflection bit mask");
  auto put_rframe = [&](int f, V3 P, V3 D, double rp) {
    if (KLR > 0 && f < KLR) {
      lds_f64* q = lf + (KL * 4 + f * 7) * 64;
      q[0] = P.x; q[64] = P.y; q[128] = P.z; q[192] = D.x; q[256] = D.y; q[320] = D.z; q[384] = rp;
    } else {
      fP[f][0] = P.x; fP[f][1] = P.y; fP[f][2] = P.z; fD[f][0] = D.x; fD[f][1] = D.y; fD[f][2] = D.z; fRP[f] = rp;
    }
  };
  auto get_rframe = [&](int f, V3* P, V3* D, double* rp) {
    if (KLR > 0 && f < KLR) {
      const lds_f64* q = lf + (KL * 4 + f * 7) * 64;
      *P = {q[0], q[64], q[128]}; *D = {q[192], q[256], q[320]}; *rp = q[384];
    } else {
      *P = {fP[f][0], fP[f][1], fP[f][2]}; *D = {fD[f][0], fD[f][1], fD[f][2]}; *rp = fRP[f];
    }
  };
  constexpr bool RECORD = !same_type<Rec, NoRec>::value;
  // Shared sphere terms (SphereShare) and constant hit filters in the refraction kernels only: at
  // 4 waves/SIMD they have the registers for them, the reflection-only megakernel spills
  // (DESIGN.md section 7).
  constexpr bool SHARE = REFR;
  constexpr bool OBB = !REFR;                          // oriented object boxes: reflection-only kernels
  int fSlot[RECORD ? RT_MAX_DEPTH_CAP : 1];
  [[maybe_unused]] int ray_type = 0, slot = 0;                  // RayType::NormalRay
  int sp = 0, depth = 0;
  Col C = {0.0, 0.0, 0.0};
  for (int iter = 0;; ++iter) {
    bool descend = false;
    [[maybe_unused]] bool pushing = false;        // POOL: this lane pushes frame `iter` (its sp) now
    [[maybe_unused]] Col push_A = {0.0, 0.0, 0.0};
    [[maybe_unused]] double push_w = 0.0;
    double t_hit;
    int oi;
    uint32_t nmask = 0xffffffffu;
    if constexpr (MASKS) {
      // `iter` and `plane_tile` are the same in every lane still here, but both are carried round a loop
      // that lanes leave one by one, so the compiler takes them for per-lane values: the choice is made on
      // their first active lane's copies, which keeps the mask (and every test on it) scalar.
      const int it = __builtin_amdgcn_readfirstlane(iter);
      const bool pt = __builtin_amdgcn_readfirstlane((int)plane_tile) != 0;
      if (it == 0) nmask = tm.w[0];
      else if (pt && it == 1) nmask = tm.w[5];
      nmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)nmask);
    }
    oi = nearest_hit<SHARE, OBB>(S, ro, rd, &t_hit, nmask);
    // depth 0: is every hit of the wave on the mask plane?  Voted here, by every lane of the iteration
    // (a lane that missed takes no part in what follows), not inside the branch of the lanes that hit.
    // (`refl` at iteration 1 rests on this flag alone: it is only ever written here, at iteration 0, which
    // no lane re-enters -- the bounce loop never restarts a pixel.  A change that lets a lane take a second
    // primary ray inside this loop must clear plane_tile with it.)
    if constexpr (MASKS)
      if (iter == 0) plane_tile = mask_plane >= 0 && __ballot(oi >= tm.hit_min && oi != mask_plane) == 0;
    const V3 p = add(ro, scale(rd, t_hit));                               // :162
    if constexpr (RECORD) slot = rec->begin(depth, ray_type, ro, rd, t_hit, oi, p);
    V3 nrm = {0.0, 0.0, 0.0};
    Col c = {0.0, 0.0, 0.0}, L = {0.0, 0.0, 0.0};
    double transp = 0.0, refl = 0.0, nlen = 0.0;
    if (oi >= 0) {
      // (k is the same in every lane, but the loop sits in the branch of the lanes that hit: the word is
      // chosen by its first-lane copy, scalar selects)
      RT_HIT_LIGHTS(
        if constexpr (MASKS)
          if (__builtin_amdgcn_readfirstlane((int)(plane_tile && iter == 0)) != 0 && k < 4) {
            const int ks = __builtin_amdgcn_readfirstlane(k);
            smask = ks == 0 ? tm.w[1] : ks == 1 ? tm.w[2] : ks == 2 ? tm.w[3] : tm.w[4];
          })
    }
    if (oi < 0) {
      C = {0.0, 0.0, 0.0};                                               // Color::BLACK (:152-160)
    } else {
      // The inside test (:230-235) only matters for a hit that spawns a ray: one with
      // depth < max_depth and a reflectivity or a transparency.  Other hits skip its division
      // and square roots (the values it would give are never read).
      bool inside = false;
      if (depth < max_depth && (refl != 0.0 || (REFR && transp != 0.0))) {
        RT_HIT_INSIDE()
      }
      const V3 n2 = inside ? scale(nrm, -1.0) : nrm;
      const double r1 = inside ? 1.45 : 1.0, r2 = inside ? 1.0 : 1.45;
      bool tir = false;
      V3 tdir = {0.0, 0.0, 0.0};
      const bool do_refr = REFR && depth < max_depth && transp != 0.0;   // :242
      if (do_refr) tdir = refract_dir(rd, n2, r1 / r2, &tir);
      const double rp = tir ? refl + (1.0 - refl) * transp : refl;       // :261-265
      const bool do_refl = depth < max_depth && rp != 0.0 && (!inside || tir);   // :267
      if constexpr (POOL) {             // one push point for both kinds of child (see pool_push)
        const bool rfr = do_refr && !tir;
        if (rfr || do_refl) {
          const double w = rfr ? transp : rp;
          push_A = intensify<FC>(L, 1.0 - w);
          push_w = w;
          pushing = true;
        }
      }
      if (do_refr && !tir) {
        if constexpr (!POOL) put_frame(sp, intensify<FC>(L, 1.0 - transp), transp);
        if constexpr (TREE) {
          pend = do_refl ? pend | (1u << sp) : pend & ~(1u << sp);
          if (do_refl) put_rframe(sp, p, reflect_dir(rd, n2), rp);
        }                                                                  // CHAIN: do_refl is false here
        if constexpr (RECORD) { fSlot[sp] = slot; ray_type = 2; }        // TransmissionRay
        ++sp;
        ro = p;
        rd = tdir;
        depth = sp;
        descend = true;
      } else if (do_refl) {
        if constexpr (!POOL) put_frame(sp, intensify<FC>(L, 1.0 - rp), rp);
        if constexpr (TREE) pend &= ~(1u << sp);
        if constexpr (RECORD) { fSlot[sp] = slot; ray_type = 1; }        // ReflectionRay
        ++sp;
        rd = reflect_dir(rd, n2);
        ro = p;
        depth = sp;
        descend = true;
      } else {
        C = L;
      }
    }
    if constexpr (RECORD) { if (!descend) rec->finish(slot, C); }     // leaf ray (or miss) reports now
    if constexpr (POOL) {                                                // frame `iter` (= sp before the push)
      if (iter < KL) {
        if (pushing) put_frame(iter, push_A, push_w);                     // the lane's own LDS slot
      } else {
        pool_push(pushing, iter, push_A, push_w, oi);
      }
    }
    if (descend) continue;
    while (sp > 0) {                                                      // post-order combine
      const int f = sp - 1;
      Col fa;
      double fw;
      get_frame(f, &fa, &fw);
      const Col comb = cadd<FC>(fa, intensify<FC>(C, fw));
      if constexpr (TREE) {
        if ((pend >> f) & 1u) {                                           // refraction done -> reflection
          pend &= ~(1u << f);
          double frp;
          get_rframe(f, &ro, &rd, &frp);
          put_frame(f, intensify<FC>(comb, 1.0 - frp), frp);
          depth = sp;
          descend = true;
          if constexpr (RECORD) ray_type = 1;                              // ReflectionRay
          break;
        }
      }
      C = comb;
      if constexpr (RECORD) rec->finish(fSlot[f], C);                  // parent reports after its children
      --sp;
    }
    if (!descend) return C;
  }
}

// ---------------------------------------------------------------- deferred shadows (REFR=false)
// get_ray_color (raytracer.rs:132-287) for scenes without a transparent object, restructured so
// a pixel's critical path is its chain of nearest hits rather than nearest hits AND every shadow
// ray in series.  Without refraction every hit spawns at most one ray (the reflection), so a
// pixel's rays form a chain and the reference's recursion computes
//     C_h = L_h                                            (no reflection spawned)
//     C_h = in_range(in_range(L_h * (1 - w_h)) + in_range(C_{h+1} * w_h))      (:267-280)
// with L_h = the ambient + per-light Lambert terms of hit h (:172-228) and C = BLACK for a ray
// that misses (:152-160).  Every L_h is a pure function of hit h and its lights' shadow
// transparencies, so the three steps run as phases of one wave:
//   1. chain:   per lane, trace the nearest-hit chain; per hit record p, the normal, the material
//               colour and the reflection weight w in the lane's arrays (every hit but possibly
//               the last spawned a reflection);
//   2. shadows: every (hit, light) shadow ray of the WHOLE WAVE is dealt densely over its 64
//               lanes through an LDS window (one round = up to 64 hits; the hits' owners write
//               their points, any lane traces any (hit, light) pair, the owners read the
//               transparencies back and form L_h in light order, :199-227);
//   3. fold:    per lane, C from the last hit back to the first, the post-order combine.
// Same operations, same order per value: bit-identical to trace<false>.  A pixel whose chain is
// 11 bounces long now waits for 11 nearest-hit traversals plus a few dense shadow rounds, not
// 11 * (1 + lights) serial traversals; lanes whose chains ended early trace other lanes' shadow
// rays instead of idling.
struct ShadowWin {                  // LDS, one per wave: 2.5 KB (RT_SH_TRCAP results per round, rt_tunables.h)
  double px[64], py[64], pz[64];
  double tr[RT_SH_TRCAP];
};

// REFR (scenes with RtDevScene::ray_chains and a transparent object): a hit spawns a refraction
// ray (weight transparency) or, on TIR or for a reflective object, a reflection ray (weight rp,
// raytracer.rs:261-265), never both, so the rays still form a chain and the same three phases
// apply; the decisions, directions and weights are trace<true, ..., CHAIN>'s, the traversals take
// the refraction kernels' template arguments (shared sphere terms, draw-order shadow walk: the
// transparency product's order is the reference's).
template <int HC, bool FC = false, bool REFR = false>
RT_FN Col trace_deferred(const DS& S, V3 ro, V3 rd, int max_depth, bool valid, ShadowWin* win) {
  constexpr bool SHARE = REFR, OBB = !REFR;
  double hP[HC][3], hN[HC][3], hC[HC][3], hW[HC];
  int nh = 0;
  bool last_spawned = false;          // the last hit spawned a reflection ray (that missed)
  // ---- phase 1: the nearest-hit chain
  if (valid) {
    for (int depth = 0;; ++depth) {
      double t_hit;
      const int oi = nearest_hit<SHARE, OBB>(S, ro, rd, &t_hit);
      if (oi < 0) break;                                                   // BLACK (:152-160)
      const V3 p = add(ro, scale(rd, t_hit));                               // :162
      V3 nrm;
      Col c;
      double transp, refl;
      shade_inputs(S, oi, p, &nrm, &c, &transp, &refl);                    // :163-170
      // inside test (:230-235), exactly as trace(): needed only if a ray may spawn
      bool inside = false;
      if (depth < max_depth && (refl != 0.0 || (REFR && transp != 0.0))) {
        const V3 nd = scale(rd, -1.0);
        inside = inside_test(dot(nd, nrm) / (len(nd) * len(nrm)));
      }
      const V3 n2 = inside ? scale(nrm, -1.0) : nrm;
      bool tir = false;
      V3 tdir = {0.0, 0.0, 0.0};
      const bool do_refr = REFR && depth < max_depth && transp != 0.0;     // :242
      const double r1 = inside ? 1.45 : 1.0, r2 = inside ? 1.0 : 1.45;
      if (do_refr) tdir = refract_dir(rd, n2, r1 / r2, &tir);
      const double rp = tir ? refl + (1.0 - refl) * transp : refl;         // :261-265
      const bool refracts = do_refr && !tir;
      const bool do_refl = !refracts && depth < max_depth && rp != 0.0 && (!inside || tir);   // :267
      hP[nh][0] = p.x; hP[nh][1] = p.y; hP[nh][2] = p.z;
      hN[nh][0] = nrm.x; hN[nh][1] = nrm.y; hN[nh][2] = nrm.z;
      hC[nh][0] = c.r; hC[nh][1] = c.g; hC[nh][2] = c.b;
      hW[nh] = refracts ? transp : rp;
      ++nh;
      last_spawned = refracts || do_refl;
      if (!last_spawned) break;
      rd = refracts ? tdir : reflect_dir(rd, n2);
      ro = p;
    }
  }
  // ---- phase 2: every shadow ray of the wave, dealt over all 64 lanes
  const int lane = __lane_id();
  const int nl = S.n_lights;
  const int hpr = nl > 0 ? (RT_SH_TRCAP / nl < 64 ? RT_SH_TRCAP / nl : 64) : 64;
  for (int next = 0;;) {
    const int pend = nh - next;
    int incl = pend;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int total = __shfl(incl, 63);
    if (total == 0) break;                                                  // wave-uniform
    const int base = incl - pend;
    const int take = base >= hpr ? 0 : (pend < hpr - base ? pend : hpr - base);
    for (int i = 0; i < take; ++i) {
      win->px[base + i] = hP[next + i][0];
      win->py[base + i] = hP[next + i][1];
      win->pz[base + i] = hP[next + i][2];
    }
    const int n_pub = total < hpr ? total : hpr;
    __syncthreads();
    const int jobs = n_pub * nl;
    for (int j = lane; j < jobs; j += 64) {                                 // :176-197
      const int h = j % n_pub, k = j / n_pub;
      const V3 p = {win->px[h], win->py[h], win->pz[h]};
      const V3 lv = sub(ld3(S.lights[k].p), p);
      win->tr[j] = shadow_transparency<SHARE, OBB, OBB>(S, p, normalized(lv), len(lv));
    }
    __syncthreads();
    for (int i = 0; i < take; ++i) {                                        // L_h in light order
      const int hh = next + i;
      const V3 p = {hP[hh][0], hP[hh][1], hP[hh][2]};
      const V3 nrm = {hN[hh][0], hN[hh][1], hN[hh][2]};
      const Col c = {hC[hh][0], hC[hh][1], hC[hh][2]};
      Col L = cmul<FC>(c, in_range<FC>(0.6, 0.6, 0.6));                             // ambient (:172)
      for (int k = 0; k < nl; ++k) {                                        // :199-227
        const double tr = win->tr[k * n_pub + base + i];
        if (tr == 0.0) continue;
        RT_REC(lt, S, lights, LIGHTS, k);
        const V3 sdir = normalized(sub(ld3(lt->p), p));
        double ang = rt_acos(dot(sdir, nrm) / (len(sdir) * len(nrm)));
        if (ang >= PI_D / 2.0) ang = PI_D - ang;
        const double inten = (ang < (PI_D / 2.0) && ang >= 0.0) ? 1.0 - (ang / (PI_D / 2.0)) : 0.0;
        const Col lc = intensify<FC>(intensify<FC>(Col{lt->col[0], lt->col[1], lt->col[2]}, inten), tr);
        L = cadd<FC>(L, cmul<FC>(c, lc));
      }
      hC[hh][0] = L.r; hC[hh][1] = L.g; hC[hh][2] = L.b;
    }
    next += take;
    __syncthreads();                                                        // the window is reused
  }
  // ---- phase 3: post-order combine, last hit first
  Col C = {0.0, 0.0, 0.0};
  for (int h = nh - 1; h >= 0; --h) {
    const Col L = {hC[h][0], hC[h][1], hC[h][2]};
    const double w = hW[h];
    C = (h == nh - 1 && !last_spawned) ? L : cadd<FC>(intensify<FC>(L, 1.0 - w), intensify<FC>(C, w));   // :278-279
  }
  return C;
}

}  // namespace
