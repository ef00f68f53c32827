// rt_wavefront.h -- what the wavefront path's two units share on the device (k_wavefront.hip: the level
// kernels; k_wf_pairs.hip: the pair path): the arena and level structs, a level's pointers, pixel slots, the
// coherence key, one ray of trace()'s loop body, the append to the next level, the wave-uniform peel loop.
// The sizes, the counter names and the level tables' field order are wf_plan.h's.
#pragma once
#include "rt_device.h"
#include "wf_plan.h"

#ifndef RT_WAVES_PER_EU_WF
#define RT_WAVES_PER_EU_WF 5             // the two kernels that shade: wf_trace_kernel, wfp_shade_kernel
#endif

struct rt_ctx;

namespace rt {

struct WfArena {
  uint8_t* base;          // level tables (wf_level)
  uint32_t* count;        // the counter block (wf_plan.h WfCount)
  uint8_t* ovf;           // per pixel slot: its tree overflowed a level
  const uint32_t* perm;   // the level being traced: slot of its i-th ray in key order (null: slot order)
  uint32_t slots, cap;    // level 0 = the pixel slots (8x8 tiles x 64), levels >= 1: cap rays each
  double klo[3], kscale[3];   // origin -> 9-bit cell per axis for the coherence keys
};
struct WfLevel {
  double *ox, *oy, *oz, *dx, *dy, *dz;   // levels >= 1: the ray
  double *Lr, *Lg, *Lb, *wt, *wr;        // hit record: L (then the folded colour), refraction / reflection weights
  int32_t *pix, *ct, *cr;                // pixel slot (levels >= 1), children's slots in level d + 1 (-1: none)
  uint32_t *key, *val;                   // levels >= 1: coherence key and slot (the sort's input pairs)
  int32_t* par;                          // levels >= 1: the object whose hit spawned the ray
};
// The pair path's arrays (k_wf_pairs.hip; wf_plan.h: WfRayLayout, WfListLayout)
struct WfPairs {
  uint32_t *key, *val;          // pairs as emitted: object, ray id (level slot, or slot * n_lights + light)
  uint32_t *key_s, *val_s;      // sorted by object
  double* tp;                   // nearest pass: the sorted pair's object's nearest accepted distance
  uint32_t* count;              // the counter block's pair block (wf_plan.h WfPairCount)
  uint32_t* bins;               // bucket-sort scratch: RT_WFP_BIN_WORDS words per sort
  uint32_t cap;
  unsigned long long* tmin;     // per ray of the level: nearest accepted distance (bits; +inf: none)
  int32_t* omin;                // per ray: the least object index at that distance (INT_MAX: none)
  double *px, *py, *pz;         // per ray: the hit point
  uint32_t *kcnt, *opq;         // per shadow ray: hits of transparency-T objects / of a zero-transparency one
  uint32_t *hkey, *hval, *hkey_s, *hperm;   // per ray: hit-point key, slot; sorted: the shadow / shading order
};

// k_wf_pairs.hip, for launch_wavefront.  wfp_level: level d of the launch through the pair path, its n_ub rays
// at most (n_dev null: exactly) enqueued on st; first: the launch's first pair level.  wfp_lists: the pair lists
// for `need` pairs (0: whatever there is), grown by wf_list_size's rule -- growing waits for their readers.
int wfp_level(rt_ctx* c, hipStream_t st, const WfPlan& plan, const WfArena& A, int d, uint32_t n_ub,
              const uint32_t* n_dev, WfRows rows, bool first);
int wfp_lists(rt_ctx* c, const WfPlan& plan, size_t need);

}  // namespace rt

namespace {

using rt::WfArena;
using rt::WfLevel;
using rt::WfPairs;
using rt::WfRows;

// Level d's table (wf_plan.h: wf_level_offset, the field order WfF64 / WfI32)
__host__ __device__ __forceinline__ WfLevel wf_level(const WfArena& A, int d) {
  using namespace rt;
  WfLevel v;
  const size_t len = d == 0 ? A.slots : A.cap;
  double* f = (double*)(A.base + wf_level_offset(A.slots, A.cap, d));
  if (d == 0) {
    v.ox = v.oy = v.oz = v.dx = v.dy = v.dz = nullptr;
    constexpr int f0 = WF_F64_0, q0 = WF_I32_0;              // level 0's first fields
    v.Lr = f + (WF_LR - f0) * len; v.Lg = f + (WF_LG - f0) * len; v.Lb = f + (WF_LB - f0) * len;
    v.wt = f + (WF_WT - f0) * len; v.wr = f + (WF_WR - f0) * len;
    int32_t* q = (int32_t*)(f + (WF_N_F64 - f0) * len);
    v.pix = nullptr; v.ct = q + (WF_CT - q0) * len; v.cr = q + (WF_CR - q0) * len;
    v.key = v.val = nullptr;
    v.par = nullptr;
  } else {
    v.ox = f + WF_OX * len; v.oy = f + WF_OY * len; v.oz = f + WF_OZ * len;
    v.dx = f + WF_DX * len; v.dy = f + WF_DY * len; v.dz = f + WF_DZ * len;
    v.Lr = f + WF_LR * len; v.Lg = f + WF_LG * len; v.Lb = f + WF_LB * len; v.wt = f + WF_WT * len; v.wr = f + WF_WR * len;
    int32_t* q = (int32_t*)(f + WF_N_F64 * len);
    v.pix = q + WF_PIX * len; v.ct = q + WF_CT * len; v.cr = q + WF_CR * len;
    v.key = (uint32_t*)(q + WF_KEY * len); v.val = (uint32_t*)(q + WF_VAL * len);
    v.par = q + WF_PAR * len;
  }
  return v;
}
// pixel slot -> (x, output row r); false outside the launch's rows / frame
__device__ __forceinline__ bool wf_pixel(const RtDevScene& S, uint32_t slot, WfRows rows, int* x, int* r, int* y) {
  tile_pixel(slot >> 6, (int)(slot & 63), S.width, x, r);
  if (*x >= S.width || *r >= rows.n_rows) return false;
  *y = band_row(*r, rows.y_first, rows.band_rows, rows.band_pitch, rows.n_rows);
  return *y < S.height;
}
// coherence key of a ray: direction octant (3 bits) above the 27-bit Morton code of its origin's
// cell (9 bits per axis over the scene's bounded extent, clamped).  Only the processing order
// depends on it, never a value.
__device__ __forceinline__ uint32_t wf_spread9(uint32_t v) {            // 9 bits -> every third bit
  v &= 511u;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t wf_key(const WfArena& A, V3 o, V3 d) {
  auto cell = [](double x, double lo, double sc) -> uint32_t {
    const double c = (x - lo) * sc;
    return c > 0.0 ? (c < 511.0 ? (uint32_t)c : 511u) : 0u;           // NaN -> 0
  };
  const uint32_t oct = (d.x < 0.0 ? 1u : 0u) | (d.y < 0.0 ? 2u : 0u) | (d.z < 0.0 ? 4u : 0u);
  return (oct << 27) | wf_spread9(cell(o.x, A.klo[0], A.kscale[0])) | (wf_spread9(cell(o.y, A.klo[1], A.kscale[1])) << 1) |
         (wf_spread9(cell(o.z, A.klo[2], A.kscale[2])) << 2);
}

// One ray of trace()'s loop body: nearest hit, the light loop (shadow rays first, then the shading
// inputs), the inside test and the refraction / reflection decisions (raytracer.rs:141-280).
// NH(&t) gives the nearest hit (object, distance), SH(k, p, sdir, dist) light k's shadow
// transparency: the traversals themselves (wf_ray) or the pair path's folded results (wfp_shade).
template <bool REFR, bool FC, class NH, class SH>
__device__ __forceinline__ void wf_ray_core(const DS& S, V3 ro, V3 rd, int depth, int max_depth, NH&& nh, SH&& sh,
                                            Col* Lo, double* wt, double* wr, bool* ch_t, bool* ch_r, V3* po, V3* dt,
                                            V3* dr) {
  *ch_t = *ch_r = false;
  *Lo = {0.0, 0.0, 0.0};
  *wt = *wr = 0.0;
  double t_hit;
  const int oi = nh(&t_hit);
  if (oi < 0) return;                                                   // Color::BLACK (:152-160)
  const V3 p = add(ro, scale(rd, t_hit));                               // :162
  V3 nrm = {0.0, 0.0, 0.0};
  Col c = {0.0, 0.0, 0.0}, L = {0.0, 0.0, 0.0};
  double transp = 0.0, refl = 0.0;
  bool have_shading = false;
#pragma unroll 1
  for (int k = 0; k < S.n_lights; ++k) {                                // :175-228, as trace()
    cptr<RtLight> lt = &S.lights[k];
    const V3 lv = sub(ld3(lt->p), p);
    double ll, ill;
    len_inv(lv, &ll, &ill);
    const V3 sdir = scale(lv, ill);
    const double t = sh(k, p, sdir, ll);
    if (!have_shading) {
      shade_inputs(S, oi, p, &nrm, &c, &transp, &refl);
      L = cmul<FC>(c, in_range<FC>(0.6, 0.6, 0.6));
      have_shading = true;
    }
    if (t == 0.0) continue;
    double ang = rt_acos(dot(sdir, nrm) / (len(sdir) * len(nrm)));
    if (ang >= PI_D / 2.0) ang = PI_D - ang;
    const double inten = (ang < (PI_D / 2.0) && ang >= 0.0) ? 1.0 - (ang / (PI_D / 2.0)) : 0.0;
    const Col lc = intensify<FC>(intensify<FC>(Col{lt->col[0], lt->col[1], lt->col[2]}, inten), t);
    L = cadd<FC>(L, cmul<FC>(c, lc));
  }
  if (!have_shading) {
    shade_inputs(S, oi, p, &nrm, &c, &transp, &refl);
    L = cmul<FC>(c, in_range<FC>(0.6, 0.6, 0.6));
  }
  bool inside = false;                                                  // :230-235
  if (depth < max_depth && (refl != 0.0 || (REFR && transp != 0.0))) {
    const V3 nd = scale(rd, -1.0);
    inside = inside_test(dot(nd, nrm) / (len(nd) * len(nrm)));
  }
  const V3 n2 = inside ? scale(nrm, -1.0) : nrm;
  const double r1 = inside ? 1.45 : 1.0, r2 = inside ? 1.0 : 1.45;
  bool tir = false;
  V3 tdir = {0.0, 0.0, 0.0};
  const bool do_refr = REFR && depth < max_depth && transp != 0.0;     // :242
  if (do_refr) tdir = refract_dir(rd, n2, r1 / r2, &tir);
  const double rp = tir ? refl + (1.0 - refl) * transp : refl;         // :261-265
  const bool do_refl = depth < max_depth && rp != 0.0 && (!inside || tir);   // :267
  *Lo = L;
  *wt = transp;
  *wr = rp;
  *ch_t = do_refr && !tir;
  *ch_r = do_refl;
  *po = p;
  *dt = tdir;
  if (do_refl) *dr = reflect_dir(rd, n2);
}

// The rays a wave's hits spawn, appended to level d + 1 (one ballot per kind, ONE atomic per
// wave: the wave's refraction children, then its reflection children, in lane order), and the hit
// record at the ray's slot j.
__device__ __forceinline__ void wf_append(const WfArena& A, const WfLevel& lv, int d, int lane, bool live, uint32_t j,
                                          int32_t pix, Col L, double wt, double wr, bool ch_t, bool ch_r, V3 p, V3 dt,
                                          V3 dr, int32_t par = -1) {
  int32_t ct = -1, cr = -1;
  const uint64_t bt = __ballot(ch_t), br = __ballot(ch_r);
  const uint32_t nt = (uint32_t)__popcll(bt), nr = (uint32_t)__popcll(br);
  if (nt + nr) {                                             // wave-uniform: d < max_depth here
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t b0 = 0;
    if (lane == 0) b0 = atomicAdd(&A.count[rt::WFC_LEVEL + d + 1], nt + nr);
    b0 = (uint32_t)__shfl((int)b0, 0);
    const WfLevel nx = wf_level(A, d + 1);
    const uint32_t st = b0 + (uint32_t)__popcll(bt & below), sr = b0 + nt + (uint32_t)__popcll(br & below);
    bool ovf = false;
    if (ch_t) {
      if (st < A.cap) {
        nx.ox[st] = p.x; nx.oy[st] = p.y; nx.oz[st] = p.z; nx.dx[st] = dt.x; nx.dy[st] = dt.y; nx.dz[st] = dt.z;
        nx.pix[st] = pix; nx.key[st] = wf_key(A, p, dt); nx.val[st] = st; nx.par[st] = par;
        ct = (int32_t)st;
      } else ovf = true;
    }
    if (ch_r) {
      if (sr < A.cap) {
        nx.ox[sr] = p.x; nx.oy[sr] = p.y; nx.oz[sr] = p.z; nx.dx[sr] = dr.x; nx.dy[sr] = dr.y; nx.dz[sr] = dr.z;
        nx.pix[sr] = pix; nx.key[sr] = wf_key(A, p, dr); nx.val[sr] = sr; nx.par[sr] = par;
        cr = (int32_t)sr;
      } else ovf = true;
    }
    if (ovf) {                                                // this pixel is re-rendered by wf_fixup_kernel
      A.ovf[pix] = 1;
      A.count[rt::WFC_OVERFLOW] = 1;
    }
  }
  if (live) {
    lv.Lr[j] = L.r; lv.Lg[j] = L.g; lv.Lb[j] = L.b; lv.wt[j] = wt; lv.wr[j] = wr;
    lv.ct[j] = ct; lv.cr[j] = cr;
  }
}

// The wave-uniform peel loop: for each distinct value of v among the lanes of `todo` (the first such lane's, then
// the first not yet served, ...), f(u) with u in a scalar register, on the `live` lanes whose v is u -- so what f
// reads of the scene by u is a scalar load.  A wave of sorted pairs sees one object, two at a run boundary.
template <class T, class F>
__device__ __forceinline__ void wf_for_each_uniform(uint64_t todo, bool live, T v, int lane, F&& f) {
  while (todo) {
    const T u = (T)__builtin_amdgcn_readlane((int)v, (int)__builtin_ctzll(todo));
    const uint64_t mine = __ballot(live && v == u);
    todo &= ~mine;
    if ((mine >> lane) & 1) f(u);
  }
}

}  // namespace
