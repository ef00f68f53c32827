// k_masks.hip -- the tile-mask pre-pass (rt_tilemask.h): one thread per 8x8 tile evaluates the mask
// predicate for a launch geometry and writes the tile's RT_TILEMASK_WORDS words to a device table that
// the specialised row kernels read with scalar loads (rt_device.h trace()).  Also the tables' slots in
// the context (rt_ctx.h MaskSlot), the read-back entry and the host evaluation of the same predicate
// (include/rt_abi.h rt_ctx_tile_masks / rt_scene_tile_masks).
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "rt_ctx.h"
#include "rt_tilemask.h"

namespace {

__global__ __launch_bounds__(64) void tile_masks_kernel(const RtTileMaskScene* __restrict__ S, int y_first, int band_rows,
                                                        int band_pitch, int n_rows, uint32_t n_tiles,
                                                        uint32_t* __restrict__ out) {
  const uint32_t tile = blockIdx.x * 64u + threadIdx.x;
  if (tile >= n_tiles) return;
  uint32_t w[RT_TILEMASK_WORDS];
  int x0, x1, y0, y1;
  if (tilemask_rect(tile, S->width, S->height, y_first, band_rows, band_pitch, n_rows, &x0, &x1, &y0, &y1))
    tilemask_eval(*S, x0, x1, y0, y1, w);
  else
    for (int k = 0; k < RT_TILEMASK_WORDS; ++k) w[k] = 0xffffffffu;      // no valid pixel: never read
  for (int k = 0; k < RT_TILEMASK_WORDS; ++k) out[(size_t)tile * RT_TILEMASK_WORDS + k] = w[k];
}

// The dispatch records of a launch (rt_blob.h RtTileRec): one thread per order entry gathers the entry's tile
// (order[e], or e without an order) from the tile-indexed mask table.
__global__ __launch_bounds__(64) void tile_records_kernel(const uint32_t* __restrict__ masks, const int32_t* __restrict__ order,
                                                          uint32_t n_entries, uint32_t n_tiles, uint32_t tiles_x,
                                                          uint32_t keep_bit, int lean_lights, uint32_t plane_bit,
                                                          RtTileRec* __restrict__ out, uint32_t* __restrict__ n_sky) {
  const uint32_t e = blockIdx.x * 64u + threadIdx.x;
  bool sky = false;
  if (e < n_entries) {
    const uint32_t tile = order ? (uint32_t)order[e] : e;
    RtTileRec r;
    r.x0 = (int32_t)((tile % tiles_x) * RT_TILE_W);
    r.r0 = (int32_t)((tile / tiles_x) * (64 / RT_TILE_W));
    for (int k = 0; k < RT_TILEMASK_WORDS; ++k)
      r.mask[k] = tile < n_tiles ? masks[(size_t)tile * RT_TILEMASK_WORDS + k] : 0xffffffffu;
    // A record whose prim word is 0 is a sky tile to the kernels (rt_device.h rows_entry).  RT_OPT_SKY_FILL 0:
    // no record says so -- an empty prim word gets the mask plane's bit, which no walk reads (the plane's
    // node ignores the mask) and which only ever makes a word looser.
    if (r.mask[0] == 0) r.mask[0] = keep_bit;
    sky = r.mask[0] == 0;
    // A lean candidate (RT_OPT_LEAN_TILES; lean_lights < 0: off): the tile is not sky, and its prim word, the
    // shadow words of the scene's lean_lights lights and its refl word hold no object but the mask plane (a word
    // the predicate gave up on is all ones).  The sign of x0 says so; the check behind this kernel
    // (launch_records) has the last word.
    bool lean = lean_lights >= 0 && !sky && tile < n_tiles && (r.mask[0] & ~plane_bit) == 0 && (r.mask[5] & ~plane_bit) == 0;
    for (int l = 0; l < lean_lights && l < 4; ++l) lean = lean && (r.mask[1 + l] & ~plane_bit) == 0;
    if (lean) r.x0 |= (int32_t)0x80000000u;
    out[e] = r;
  }
  const unsigned long long b = __ballot(sky);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_sky, (uint32_t)__popcll(b));
}

// The entries of a checked record table that kept the lean bit, counted as the gather counts the sky entries
// (atomics per wave of 64 entries): out[0] their number, out[1] the maximum of ~e, out[2] the maximum of e + 1
// (zeroed by the caller: the run [~out[1], out[2]) holds them all).  n_sky (a traced table, whose pass makes sky
// entries the gather did not count; zeroed by the caller): the entries whose prim word is empty.
__global__ __launch_bounds__(64) void lean_count_kernel(const RtTileRec* __restrict__ recs, uint32_t n_entries,
                                                        uint32_t* __restrict__ out, uint32_t* __restrict__ n_sky) {
  const uint32_t e = blockIdx.x * 64u + threadIdx.x;
  const bool lean = e < n_entries && recs[e].x0 < 0;
  const unsigned long long s = __ballot(n_sky && e < n_entries && recs[e].mask[0] == 0);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(n_sky, (uint32_t)__popcll(s));
  const unsigned long long b = __ballot(lean);
  if ((threadIdx.x & 63) == 0 && b) {
    const uint32_t base = blockIdx.x * 64u;
    atomicAdd(out, (uint32_t)__popcll(b));
    atomicMax(out + 1, ~(base + (uint32_t)__builtin_ctzll(b)));
    atomicMax(out + 2, base + 64u - (uint32_t)__builtin_clzll(b));
  }
}

bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// ---- tighter bounds of an object's accepted hits (rt_tilemask.h "vertex sets" and "ball")
// The inverse of the 3x3 part of a leaf's inverse transform, in long double as scene.cpp leaf_box has it.
bool invert3(const double* M, long double Ai[3][3]) {
  long double A[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = M[4 * i + j];
  const long double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                          A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  if (!(fabsl(det) > 1e-300L) || !std::isfinite((double)det)) return false;
  Ai[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
  Ai[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
  Ai[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
  Ai[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
  Ai[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
  Ai[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
  Ai[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
  Ai[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
  Ai[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
  return true;
}

// The world point the leaf's inverse transform takes to the local point q.  False unless it is finite, within
// the culling range, and M w + b gives q back within a quarter of scene.cpp obb()'s margin: the hull of a
// box's 8 such points then still holds the box with three quarters of the margin, a hundred times the
// rounding the margin was sized for.
bool to_world(const double* M, const long double Ai[3][3], const double q[3], double w[3]) {
  long double c[3];
  for (int i = 0; i < 3; ++i) c[i] = (long double)q[i] - M[4 * i + 3];
  for (int i = 0; i < 3; ++i) {
    w[i] = (double)(Ai[i][0] * c[0] + Ai[i][1] * c[1] + Ai[i][2] * c[2]);
    if (!(fabs(w[i]) <= RT_CULL_COORD_MAX)) return false;
  }
  for (int i = 0; i < 3; ++i) {
    const double back = M[4 * i] * w[0] + M[4 * i + 1] * w[1] + M[4 * i + 2] * w[2] + M[4 * i + 3];
    const double mi = fabs(M[4 * i]) + fabs(M[4 * i + 1]) + fabs(M[4 * i + 2]);
    if (!(fabs(back - q[i]) <= 2.5e-7 * (1.0 + mi))) return false;
  }
  return true;
}

bool box_to_world(const double* M, const long double Ai[3][3], const double lo[3], const double hi[3], double W[8][3]) {
  for (int k = 0; k < 8; ++k) {
    const double q[3] = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
    if (!to_world(M, Ai, q, W[k])) return false;
  }
  return true;
}

// Object o's vertex sets and ball.  Every leaf scene.cpp obb() would accept as required (one test,
// rt::required_leaf_box) bounds all accepted hits by its inflated local box, taken to world space as 8
// corners; each box is first cut down, in its own frame, to the extent the other required leaves' world
// corners have there (hits lie in every one of those hulls; 1e-9 relative for the transform's rounding) --
// globes.scene's rods are a thin long sphere inside a cube: 2 x 200 x 2 becomes 2 x 40 x 2.  A required sphere
// leaf whose transform is a similarity (rows orthogonal and of one length within 1e-9) also gives a ball:
// |M p + b - c| <= r_eps means |p - centre| <= r_eps / scale.
void object_bounds(const rt::FlatScene& f, const RtObject& ob, int o, RtTileMaskScene* t, int* n_sets) {
  struct Req {
    const RtLeaf* R;
    long double Ai[3][3];
    double lo[3], hi[3], W[8][3];
  };
  std::vector<Req> req;
  for (int32_t r = ob.leaf_begin; r < ob.leaf_begin + ob.leaf_count && req.size() < RT_TILEMASK_OBJ_SETS; ++r) {
    Req q;
    double det;
    q.R = &f.leaves[(size_t)r];
    if (!rt::required_leaf_box(f, ob, r, q.lo, q.hi, &det) || !invert3(q.R->inv, q.Ai)) continue;
    if (!box_to_world(q.R->inv, q.Ai, q.lo, q.hi, q.W)) continue;
    req.push_back(q);
  }
  double best_r2 = INFINITY;
  for (size_t a = 0; a < req.size(); ++a) {
    const Req& q = req[a];
    const double* M = q.R->inv;
    // ---- the ball
    if (q.R->kind == RT_N_SPHERE) {
      double G[3][3], w[3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = M[4 * i] * M[4 * j] + M[4 * i + 1] * M[4 * j + 1] + M[4 * i + 2] * M[4 * j + 2];
      const double s2 = (G[0][0] + G[1][1] + G[2][2]) / 3.0;
      bool sim = std::isfinite(s2) && s2 > 1e-200 && s2 < 1e200;
      for (int i = 0; i < 3 && sim; ++i)
        for (int j = 0; j < 3 && sim; ++j) sim = fabs(G[i][j] - (i == j ? s2 : 0.0)) <= 1e-9 * s2;
      if (sim && to_world(M, q.Ai, q.R->c, w)) {
        double rl = 0.0;                                    // r_eps plus obb()'s margin, the widest axis
        for (int i = 0; i < 3; ++i) rl = fmax(rl, 0.5 * (q.hi[i] - q.lo[i]));
        const double wmax = fmax(fmax(fabs(w[0]), fabs(w[1])), fabs(w[2]));
        const double rw = rl / sqrt(s2) * (1.0 + 1e-6) + 1e-6 * (1.0 + wmax), r2 = rw * rw;
        if (std::isfinite(r2) && r2 < best_r2) {
          best_r2 = r2;
          for (int i = 0; i < 3; ++i) t->ball[o][i] = w[i];
          t->ball[o][3] = r2;
          t->balled |= 1u << o;
        }
      }
    }
    // ---- the vertex set: the leaf's box cut down to the others' extent in its frame
    if (*n_sets >= RT_TILEMASK_SETS) continue;
    double lo[3], hi[3];
    bool ok = true;
    for (int i = 0; i < 3; ++i) { lo[i] = q.lo[i]; hi[i] = q.hi[i]; }
    for (size_t b = 0; b < req.size() && ok; ++b) {
      if (b == a) continue;
      for (int i = 0; i < 3 && ok; ++i) {
        double l = INFINITY, h = -INFINITY;
        for (int k = 0; k < 8; ++k) {
          const double* w = req[b].W[k];
          const double v = M[4 * i] * w[0] + M[4 * i + 1] * w[1] + M[4 * i + 2] * w[2] + M[4 * i + 3];
          // the transform's rounding, and to_world's residual on the cut face four times over
          const double m = 1e-9 * (1.0 + fabs(M[4 * i] * w[0]) + fabs(M[4 * i + 1] * w[1]) + fabs(M[4 * i + 2] * w[2]) + fabs(M[4 * i + 3])) +
                           1e-6 * (1.0 + fabs(M[4 * i]) + fabs(M[4 * i + 1]) + fabs(M[4 * i + 2]));
          l = fmin(l, v - m);
          h = fmax(h, v + m);
          ok = ok && std::isfinite(v) && std::isfinite(m);
        }
        lo[i] = fmax(lo[i], l);
        hi[i] = fmin(hi[i], h);
        ok = ok && lo[i] <= hi[i];
      }
    }
    double W[8][3];
    if (!ok || !box_to_world(M, q.Ai, lo, hi, W)) memcpy(W, q.W, sizeof W);      // the uncut box is a bound too
    memcpy(t->sets[*n_sets], W, sizeof W);
    ++*n_sets;
  }
}

// What the predicate reads of a flattened scene.  valid = 0 (every word all ones) for scenes of more than
// RT_TILEMASK_OBJECTS objects, frames beyond RT_TILEMASK_MAX_SIDE and non-finite cameras.
void tilemask_scene(const rt::FlatScene& f, RtTileMaskScene* t) {
  memset((void*)t, 0, sizeof *t);
  t->cam = f.cam;
  t->width = f.width;
  t->height = f.height;
  t->n_objects = (int32_t)f.objects.size();
  t->n_lights = (int32_t)f.lights.size();
  t->plane = -1;
  const RtCamera& cam = f.cam;
  t->valid = f.objects.size() <= RT_TILEMASK_OBJECTS && f.width >= 1 && f.height >= 1 && f.width <= RT_TILEMASK_MAX_SIDE &&
             f.height <= RT_TILEMASK_MAX_SIDE && finite3(cam.center) && finite3(cam.direction) && finite3(cam.right) &&
             finite3(cam.up) && std::isfinite(cam.aspect) && cam.width > 0.0 && cam.height > 0.0;
  if (!t->valid) {
    t->n_objects = 0;
    return;
  }
  int n_sets = 0;
  for (size_t o = 0; o < f.objects.size(); ++o) {
    const RtObject& ob = f.objects[o];
    bool boxed = ob.cull == RT_CULL_BOX;
    for (int k = 0; k < 3; ++k) {
      t->blo[o][k] = ob.blo[k];
      t->bhi[o][k] = ob.bhi[k];
      boxed = boxed && fabs(ob.blo[k]) <= RT_CULL_COORD_MAX && fabs(ob.bhi[k]) <= RT_CULL_COORD_MAX && ob.blo[k] <= ob.bhi[k];
    }
    if (boxed) t->boxed |= 1u << o;
    t->set_begin[o] = n_sets;
    if (boxed) object_bounds(f, ob, (int)o, t, &n_sets);
  }
  for (size_t o = f.objects.size(); o <= RT_TILEMASK_OBJECTS; ++o) t->set_begin[o] = n_sets;
  for (int l = 0; l < t->n_lights && l < RT_TILEMASK_LIGHTS; ++l)
    for (int k = 0; k < 3; ++k) t->light[l][k] = f.lights[(size_t)l].p[k];
  t->plane = rt::tilemask_plane(f);
  if (t->plane < 0) return;
  // the plane in world space, as leaf_candidates meets it: pnorm . (inv x) + d = 0 (rt_device.h)
  const RtObject& ob = f.objects[(size_t)t->plane];
  const RtLeaf& L = f.leaves[(size_t)ob.leaf_begin];
  for (int j = 0; j < 3; ++j) t->pn[j] = L.pnorm[0] * L.inv[j] + L.pnorm[1] * L.inv[4 + j] + L.pnorm[2] * L.inv[8 + j];
  t->pd = L.pnorm[0] * L.inv[3] + L.pnorm[1] * L.inv[7] + L.pnorm[2] * L.inv[11] + L.pl[0][3];
  const double pl = sqrt(t->pn[0] * t->pn[0] + t->pn[1] * t->pn[1] + t->pn[2] * t->pn[2]);
  if (!(std::isfinite(pl) && pl > 1e-100 && pl < 1e100 && std::isfinite(t->pd))) {
    t->plane = -1;
    return;
  }
  // refl: the shading normal the reflection mirrors in (RtObject::nunit) must be the geometric one
  const double u[3] = {t->pn[0] / pl, t->pn[1] / pl, t->pn[2] / pl}, *m = ob.nunit;
  const double cx = u[1] * m[2] - u[2] * m[1], cy = u[2] * m[0] - u[0] * m[2], cz = u[0] * m[1] - u[1] * m[0];
  t->refl_ok = fabs(ob.nunit_len - 1.0) <= 1e-12 && sqrt(cx * cx + cy * cy + cz * cz) <= 1e-12;
}

void drop_mask(rt_ctx::MaskSlot& s) {
  if (s.d_masks) (void)hipFree(s.d_masks);       // hipFree waits for work that may still read it
  if (s.ready) (void)hipEventDestroy(s.ready);
  s = rt_ctx::MaskSlot();
}

void drop_rec(rt_ctx::RecSlot& s) {
  if (s.d_recs) (void)hipFree(s.d_recs);         // hipFree waits for work that may still read it
  if (s.h_sky) (void)hipHostFree(s.h_sky);
  if (s.ready) (void)hipEventDestroy(s.ready);
  s = rt_ctx::RecSlot();
}

}  // namespace

namespace rt {

int mask_slot(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, size_t n_tiles, rt_ctx::MaskSlot** out) {
  const int32_t key[5] = {a0, a1, a2, a3, c->dev.width};
  bool found;
  rt_ctx::MaskSlot* slot = find_slot(c->masks, [&](const rt_ctx::MaskSlot& s) { return memcmp(s.key, key, sizeof key) == 0; }, &found);
  if (!found) {
    drop_mask(*slot);
    RT_HIP(hipMalloc((void**)&slot->d_masks, n_tiles * RT_TILEMASK_WORDS * sizeof(uint32_t)));
    RT_HIP(hipEventCreateWithFlags(&slot->ready, hipEventDisableTiming));
    memcpy(slot->key, key, sizeof key);
    slot->n_tiles = n_tiles;
    hipLaunchKernelGGL(tile_masks_kernel, dim3((unsigned)((n_tiles + 63) / 64)), dim3(64), 0, st,
                       (const RtTileMaskScene*)c->d_mask_scene, a0, a1, a2, a3, (uint32_t)n_tiles, slot->d_masks);
    RT_HIP(hipGetLastError());
    RT_HIP(hipEventRecord(slot->ready, st));
    slot->fill_stream = st;
    slot->fill_id = ++c->mask_fills;
    slot->valid = true;
  }
  slot->last_use = ++c->use_clock;
  *out = slot;
  return wait_ready(*slot, st);       // another stream's launch: after the fill
}

void drop_masks(rt_ctx* c) {
  for (auto& s : c->masks) drop_mask(s);
  drop_records(c);                     // gathered from them
}

void drop_records(rt_ctx* c) {
  for (auto& s : c->recs) drop_rec(s);
}

// The mask plane: the first object in draw order that is one plane leaf whose constant unit normal the
// host formed (RtObject::unit_normal); the specialised program holds the same index (spec_text.cpp MASK_PLANE).
int tilemask_plane(const FlatScene& f) {
  if (f.objects.size() > RT_TILEMASK_OBJECTS) return -1;
  for (size_t o = 0; o < f.objects.size(); ++o) {
    const RtObject& ob = f.objects[o];
    if (ob.node_count == 1 && ob.leaf_count == 1 && ob.unit_normal && f.leaves[(size_t)ob.leaf_begin].kind == RT_N_PLANE)
      return (int)o;
  }
  return -1;
}

// Sky tiles (RT_OPT_SKY_FILL): a tile's prim word can only be 0 -- no primary ray of the tile hits anything,
// every pixel BLACK -- when every object is boxed or is the mask plane (an unbounded object keeps its bit);
// the specialised programs compile the early-out in for such scenes only (spec_text.cpp SKY_OK).
bool tilemask_sky_ok(const FlatScene& f) {
  const int plane = tilemask_plane(f);
  if (plane < 0) return false;
  for (size_t o = 0; o < f.objects.size(); ++o)
    if ((int)o != plane && f.objects[o].cull != RT_CULL_BOX) return false;
  return true;
}

// Lean tiles (RT_OPT_LEAN_TILES): a record may say lean only where the mask plane is the one unbounded object
// (every walk under a word without boxed objects then visits the plane alone) and the record's four shadow
// words cover the scene's lights; the specialised programs hold the kernels for such scenes only (LEAN_OK).
bool tilemask_lean_ok(const FlatScene& f) {
  return tilemask_sky_ok(f) && !f.any_transparent && f.lights.size() <= RT_TILEMASK_LIGHTS;
}

// rt_scene_describe's lines on the tile masks' bounds: per boxed object its vertex sets and whether it has a ball
std::string describe_tile_bounds(const FlatScene& f) {
  RtTileMaskScene t;
  tilemask_scene(f, &t);
  std::string s;
  char buf[128];
  for (int o = 0; o < t.n_objects; ++o) {
    if (!((t.boxed >> o) & 1u)) continue;
    snprintf(buf, sizeof buf, "tile-mask bounds object %d: sets %d ball %d\n", o, t.set_begin[o + 1] - t.set_begin[o],
             (int)((t.balled >> o) & 1u));
    s += buf;
  }
  return s;
}

size_t put_mask_scene(const FlatScene& f, std::vector<uint8_t>& blob, bool* ok) {
  RtTileMaskScene t;
  tilemask_scene(f, &t);
  *ok = t.valid != 0;
  const size_t off = (blob.size() + 255) & ~(size_t)255;
  blob.resize(off + sizeof t + 16);
  memcpy(blob.data() + off, &t, sizeof t);
  return off;
}

bool masks_usable(const rt_ctx* c) {
  static const bool off = diag_env("RT_NO_TILE_MASKS");
  return c->masks_ok && !off;
}

// The record table of a masked launch: found by the mask fill it read and the calibration that wrote its order
// (a table of an earlier fill -- the masks are dropped on every upload -- or of another order is never taken),
// else gathered on st, behind the mask fill: mask_slot has put the fill, or a wait for its event, on st
// already.  Launches on other streams wait for the gather's own event.
int launch_records(rt_ctx* c, hipStream_t st, const rt_ctx::MaskSlot* ms, const int32_t* d_order, uint64_t order_id,
                   uint32_t n_entries, bool lean, int traced, const RtTileRec** table, const void** rslot) {
  *table = nullptr;
  if (rslot) *rslot = nullptr;
  const bool sky_fill = c->sky_fill && c->sky_ok;
  bool found;
  rt_ctx::RecSlot* slot = find_slot(c->recs, [&](const rt_ctx::RecSlot& s) {
    return s.fill_id == ms->fill_id && s.order_id == order_id && s.n_entries == n_entries && s.sky_fill == sky_fill &&
           s.lean == lean && s.traced == traced;
  }, &found);
  if (!found) {
    drop_rec(*slot);
    // (one more record's room behind the table: the counts of sky and lean entries, for rt_ctx_kernel_info, and
    // the lean entries' run, for their kernel's grid)
    RT_HIP(hipMalloc((void**)&slot->d_recs, ((size_t)n_entries + 1) * sizeof(RtTileRec)));
    slot->d_sky = (uint32_t*)(slot->d_recs + n_entries);
    RT_HIP(hipMemsetAsync(slot->d_sky, 0, 4 * sizeof(uint32_t), st));
    RT_HIP(hipHostMalloc((void**)&slot->h_sky, 4 * sizeof(uint32_t), hipHostMallocDefault));
    memset(slot->h_sky, 0, 4 * sizeof(uint32_t));
    slot->lean = lean;
    slot->traced = traced;
    slot->rec_id = ++c->rec_ids;
    slot->sky_fill = sky_fill;
    RT_HIP(hipEventCreateWithFlags(&slot->ready, hipEventDisableTiming));
    slot->order_id = order_id;
    slot->fill_id = ms->fill_id;
    slot->n_entries = n_entries;
    const uint32_t tiles_x = (uint32_t)((c->dev.width + RT_TILE_W - 1) / RT_TILE_W);
    const uint32_t keep_bit = sky_fill || c->mask_plane < 0 ? 0u : 1u << c->mask_plane;   // what an empty prim word gets
    hipLaunchKernelGGL(tile_records_kernel, dim3((n_entries + 63) / 64), dim3(64), 0, st, (const uint32_t*)ms->d_masks, d_order,
                       n_entries, (uint32_t)ms->n_tiles, tiles_x,
                       keep_bit, lean && !traced ? c->dev.n_lights : -1,
                       c->mask_plane < 0 ? 0u : 1u << c->mask_plane, slot->d_recs, slot->d_sky);
    RT_HIP(hipGetLastError());
    if (lean || traced) {
      // the check (rt_bodies.h lean_check_body): the program's own kernel over every entry, behind the gather;
      // it clears the bit where a reflected ray would hit; the entries that keep it are counted behind it.
      // traced: the trace pass in its place (mode bit 0; bit 1: entries may say lean) -- the gather sets no
      // candidate bits, the pass sets the lean bits and makes more sky entries, so the sky count is taken again
      // with the lean count.  Mode bit 2: the entries with a pixel on a boxed object are traced too (form 2).
      const int a0 = ms->key[0], a1 = ms->key[1], a2 = ms->key[2], a3 = ms->key[3];
      const int mode = traced ? (lean ? 3 : 1) | (traced == 2 ? 4 : 0) : 0;
      RtTileRec* d_recs = slot->d_recs;
      void* kargs[] = {&c->dev, (void*)&a0, (void*)&a1, (void*)&a2, (void*)&a3, &d_recs, (void*)&mode, (void*)&keep_bit};
      RT_HIP(hipModuleLaunchKernel(spec_fn(c, SPEC_LEAN_CHECK, false, false), n_entries, 1, 1, 64, 1, 1, 0, st, kargs, nullptr));
      if (traced) RT_HIP(hipMemsetAsync(slot->d_sky, 0, sizeof(uint32_t), st));
      hipLaunchKernelGGL(lean_count_kernel, dim3((n_entries + 63) / 64), dim3(64), 0, st, (const RtTileRec*)slot->d_recs, n_entries,
                         slot->d_sky + 1, traced ? slot->d_sky : (uint32_t*)nullptr);
      RT_HIP(hipGetLastError());
    }
    RT_HIP(hipMemcpyAsync(slot->h_sky, slot->d_sky, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RT_HIP(hipEventRecord(slot->ready, st));
    slot->fill_stream = st;
    slot->valid = true;
  }
  slot->last_use = ++c->use_clock;
  *table = slot->d_recs;
  if (rslot) *rslot = slot;
  return wait_ready(*slot, st);       // another stream's launch: after the gather
}

uint64_t record_id(const void* rslot) { return rslot ? ((const rt_ctx::RecSlot*)rslot)->rec_id : 0; }

// The sky entries among a record table's (rt_ctx_kernel_info): the pinned word the gather's stream copied the
// count to, read once the gather's event has completed -- no wait, no stream touched.
int64_t record_sky_entries(rt_ctx* c, const void* rslot, uint64_t rec_id, uint32_t* n_entries) {
  const rt_ctx::RecSlot* slot = (const rt_ctx::RecSlot*)rslot;
  if (!slot || !slot->valid || slot->rec_id != rec_id) return -1;
  if (!slot->seen_ready && hipEventQuery(slot->ready) != hipSuccess) {
    (void)hipGetLastError();
    return -2;
  }
  *n_entries = slot->n_entries;
  return (int64_t)*slot->h_sky;
}

// The same for the entries that say lean once the table's check has run (a table gathered without them: 0).
int64_t record_lean_entries(rt_ctx* c, const void* rslot, uint64_t rec_id) {
  uint32_t n = 0;
  const int64_t rc = record_sky_entries(c, rslot, rec_id, &n);
  return rc < 0 ? rc : (int64_t)((const rt_ctx::RecSlot*)rslot)->h_sky[1];
}

bool record_lean_range(const void* rslot, uint32_t* first, uint32_t* end) {
  rt_ctx::RecSlot* slot = (rt_ctx::RecSlot*)rslot;     // (the launch's own slot, as launch_records gave it)
  if (!slot || !slot->valid || !slot->lean) return false;
  if (!slot->seen_ready) {
    if (hipEventQuery(slot->ready) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    slot->seen_ready = true;
  }
  const uint32_t n = slot->h_sky[1], lo = ~slot->h_sky[2], hi = slot->h_sky[3];
  if (n == 0) { *first = *end = 0; return true; }
  if (!(lo < hi && hi <= slot->n_entries)) return false;   // (never: the words are this table's)
  *first = lo;
  *end = hi;
  return true;
}

}  // namespace rt

extern "C" {

int rt_ctx_tile_masks(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                      uint32_t* words, size_t cap_words, uint32_t* n_tiles_out) {
  if (!c || !n_tiles_out || (cap_words > 0 && !words)) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (c->views.kind) return fail(RT_ERR_UNSUPPORTED, "rt_ctx_tile_masks is not built for a two-eye scene (stereoscopic / anaglyph camera)");
  const rt::BandGeometry g = rt::band_geometry(c->dev.width, c->dev.height, y_first, band_rows, band_pitch, n_bands);
  if (g.status != rt::BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  const size_t n_tiles = g.n_tiles;
  *n_tiles_out = (uint32_t)n_tiles;
  const size_t n = std::min(cap_words, n_tiles * RT_TILEMASK_WORDS);
  if (n == 0) return RT_OK;
  if (!c->masks_ok) {                                        // a scene the kernels take no masks for: all ones
    for (size_t i = 0; i < n; ++i) words[i] = 0xffffffffu;
    return RT_OK;
  }
  RT_HIP(hipSetDevice(c->device));
  rt_ctx::MaskSlot* slot = nullptr;
  RT_TRY(rt::mask_slot(c, nullptr, (int)y_first, (int)band_rows, (int)band_pitch, (int)g.n_rows, n_tiles, &slot));
  RT_HIP(hipStreamSynchronize(nullptr));
  RT_HIP(hipMemcpy(words, slot->d_masks, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_ctx_tile_records(rt_ctx* c, uint32_t* words, size_t cap_entries, uint32_t* n_entries) {
  if (!c || !n_entries || (cap_entries > 0 && !words)) return fail(RT_ERR_INVALID, "null argument");
  static_assert(sizeof(RtTileRec) == 8 * sizeof(uint32_t), "a record is 8 words");
  const rt_ctx::RecSlot* slot = (const rt_ctx::RecSlot*)c->last_rec_slot;
  if (!slot || !slot->valid || slot->rec_id != c->last_rec_id)
    return fail(RT_ERR_INVALID, "the last row launch read no dispatch records (or their table has been dropped)");
  RT_HIP(hipSetDevice(c->device));
  RT_HIP(hipEventSynchronize(slot->ready));
  *n_entries = slot->n_entries;
  const size_t n = std::min(cap_entries, (size_t)slot->n_entries);
  if (n) RT_HIP(hipMemcpy(words, slot->d_recs, n * sizeof(RtTileRec), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_scene_tile_masks(const rt_scene* s, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                        uint32_t* words, size_t cap_words, int32_t info[4]) {
  if (!s || !info || (cap_words > 0 && !words)) return fail(RT_ERR_INVALID, "null argument");
  if (s->cam_kind != RT_CAMERA_PERSPECTIVE)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_tile_masks is not built for a two-eye scene (stereoscopic / anaglyph camera)");
  rt::FlatScene f;
  RT_TRY(rt::flatten(*s, &f));
  const rt::BandGeometry g = rt::band_geometry(f.width, f.height, y_first, band_rows, band_pitch, n_bands);
  if (g.status != rt::BandGeometry::OK) return fail(RT_ERR_INVALID, "%s", g.error);
  const size_t n_tiles = g.n_tiles;
  RtTileMaskScene t;
  tilemask_scene(f, &t);
  info[0] = (int32_t)n_tiles;
  info[1] = t.plane;
  info[2] = (int32_t)t.boxed;
  info[3] = t.valid;
  for (size_t tile = 0; tile < n_tiles && (tile + 1) * RT_TILEMASK_WORDS <= cap_words; ++tile) {
    uint32_t* w = words + tile * RT_TILEMASK_WORDS;
    int x0, x1, y0, y1;
    if (tilemask_rect((unsigned)tile, f.width, f.height, (int)y_first, (int)band_rows, (int)band_pitch, (int)g.n_rows, &x0, &x1, &y0, &y1))
      tilemask_eval(t, x0, x1, y0, y1, w);
    else
      for (int k = 0; k < RT_TILEMASK_WORDS; ++k) w[k] = 0xffffffffu;
  }
  return RT_OK;
}

}  // extern "C"
