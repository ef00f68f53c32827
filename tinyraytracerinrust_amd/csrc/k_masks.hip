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
                                                          RtTileRec* __restrict__ out) {
  const uint32_t e = blockIdx.x * 64u + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t tile = order ? (uint32_t)order[e] : e;
  RtTileRec r;
  r.x0 = (int32_t)((tile % tiles_x) * RT_TILE_W);
  r.r0 = (int32_t)((tile / tiles_x) * (64 / RT_TILE_W));
  for (int k = 0; k < RT_TILEMASK_WORDS; ++k)
    r.mask[k] = tile < n_tiles ? masks[(size_t)tile * RT_TILEMASK_WORDS + k] : 0xffffffffu;
  out[e] = r;
}

bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

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
  for (size_t o = 0; o < f.objects.size(); ++o) {
    const RtObject& ob = f.objects[o];
    bool boxed = ob.cull == RT_CULL_BOX;
    for (int k = 0; k < 3; ++k) {
      t->blo[o][k] = ob.blo[k];
      t->bhi[o][k] = ob.bhi[k];
      boxed = boxed && fabs(ob.blo[k]) <= RT_CULL_COORD_MAX && fabs(ob.bhi[k]) <= RT_CULL_COORD_MAX && ob.blo[k] <= ob.bhi[k];
    }
    if (boxed) t->boxed |= 1u << o;
  }
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
  if (s.ready) (void)hipEventDestroy(s.ready);
  s = rt_ctx::RecSlot();
}

// Geometry of a band launch as launch_bands computes it
int mask_geometry(int width, int height, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                  int* n_rows, size_t* n_tiles) {
  if (band_rows == 0 || n_bands == 0) return fail(RT_ERR_INVALID, "no rows");
  if (band_pitch < band_rows && n_bands > 1) return fail(RT_ERR_INVALID, "band pitch %u < band rows %u", band_pitch, band_rows);
  if (y_first >= (uint32_t)height) return fail(RT_ERR_INVALID, "first row %u >= height %d", y_first, height);
  const uint64_t rows = (uint64_t)band_rows * n_bands;
  if (rows > (1u << 24)) return fail(RT_ERR_INVALID, "too many rows");
  *n_rows = (int)rows;
  const int tiles_x = (width + RT_TILE_W - 1) / RT_TILE_W, tile_h = 64 / RT_TILE_W;
  *n_tiles = (size_t)tiles_x * (size_t)((rows + tile_h - 1) / tile_h);
  return RT_OK;
}

// The slot of a geometry, filled on st if it is new since the upload
int mask_slot(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, size_t n_tiles, rt_ctx::MaskSlot** out) {
  const int32_t key[5] = {a0, a1, a2, a3, c->dev.width};
  rt_ctx::MaskSlot* slot = nullptr;
  for (auto& s : c->masks)
    if (s.valid && memcmp(s.key, key, sizeof key) == 0) slot = &s;
  if (!slot) {
    slot = &c->masks[0];
    for (auto& s : c->masks) {
      if (!s.valid) { slot = &s; break; }
      if (s.last_use < slot->last_use) slot = &s;
    }
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
  if (!slot->seen_ready && slot->fill_stream != st) {      // another stream's launch: after the fill
    if (hipEventQuery(slot->ready) == hipSuccess) {
      slot->seen_ready = true;
    } else {
      (void)hipGetLastError();
      RT_HIP(hipStreamWaitEvent(st, slot->ready, 0));
    }
  }
  *out = slot;
  return RT_OK;
}

}  // namespace

namespace rt {

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

size_t put_mask_scene(const FlatScene& f, std::vector<uint8_t>& blob, bool* ok) {
  RtTileMaskScene t;
  tilemask_scene(f, &t);
  *ok = t.valid != 0;
  const size_t off = (blob.size() + 255) & ~(size_t)255;
  blob.resize(off + sizeof t + 16);
  memcpy(blob.data() + off, &t, sizeof t);
  return off;
}

int launch_masks(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, size_t n_tiles, const uint32_t** table,
                 const void** mslot) {
  *table = nullptr;
  if (mslot) *mslot = nullptr;
  if (!c->tile_masks || !c->masks_ok) return RT_OK;
  static const bool off = diag_env("RT_NO_TILE_MASKS");
  if (off) return RT_OK;
  rt_ctx::MaskSlot* slot = nullptr;
  RT_TRY(mask_slot(c, st, a0, a1, a2, a3, n_tiles, &slot));
  *table = slot->d_masks;
  if (mslot) *mslot = slot;
  return RT_OK;
}

// The record table of a masked launch: found by the mask fill it read and the calibration that wrote its order
// (a table of an earlier fill -- the masks are dropped on every upload -- or of another order is never taken),
// else gathered on st, behind the mask fill: launch_masks has put the fill, or a wait for its event, on st
// already.  Launches on other streams wait for the gather's own event.
int launch_records(rt_ctx* c, hipStream_t st, const void* mask_slot, const int32_t* d_order, uint64_t order_id,
                   uint32_t n_entries, const RtTileRec** table) {
  const rt_ctx::MaskSlot* ms = (const rt_ctx::MaskSlot*)mask_slot;
  *table = nullptr;
  rt_ctx::RecSlot* slot = nullptr;
  for (auto& s : c->recs)
    if (s.valid && s.fill_id == ms->fill_id && s.order_id == order_id && s.n_entries == n_entries) slot = &s;
  if (!slot) {
    slot = &c->recs[0];
    for (auto& s : c->recs) {
      if (!s.valid) { slot = &s; break; }
      if (s.last_use < slot->last_use) slot = &s;
    }
    drop_rec(*slot);
    RT_HIP(hipMalloc((void**)&slot->d_recs, (size_t)n_entries * sizeof(RtTileRec)));
    RT_HIP(hipEventCreateWithFlags(&slot->ready, hipEventDisableTiming));
    slot->order_id = order_id;
    slot->fill_id = ms->fill_id;
    slot->n_entries = n_entries;
    const uint32_t tiles_x = (uint32_t)((c->dev.width + RT_TILE_W - 1) / RT_TILE_W);
    hipLaunchKernelGGL(tile_records_kernel, dim3((n_entries + 63) / 64), dim3(64), 0, st, (const uint32_t*)ms->d_masks, d_order,
                       n_entries, (uint32_t)ms->n_tiles, tiles_x, slot->d_recs);
    RT_HIP(hipGetLastError());
    RT_HIP(hipEventRecord(slot->ready, st));
    slot->fill_stream = st;
    slot->valid = true;
  }
  slot->last_use = ++c->use_clock;
  if (!slot->seen_ready && slot->fill_stream != st) {      // another stream's launch: after the gather
    if (hipEventQuery(slot->ready) == hipSuccess) {
      slot->seen_ready = true;
    } else {
      (void)hipGetLastError();
      RT_HIP(hipStreamWaitEvent(st, slot->ready, 0));
    }
  }
  *table = slot->d_recs;
  return RT_OK;
}

}  // namespace rt

extern "C" {

int rt_ctx_tile_masks(rt_ctx* c, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                      uint32_t* words, size_t cap_words, uint32_t* n_tiles_out) {
  if (!c || !n_tiles_out || (cap_words > 0 && !words)) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (c->views.kind) return fail(RT_ERR_UNSUPPORTED, "rt_ctx_tile_masks is not built for a two-eye scene (stereoscopic / anaglyph camera)");
  int n_rows = 0;
  size_t n_tiles = 0;
  RT_TRY(mask_geometry(c->dev.width, c->dev.height, y_first, band_rows, band_pitch, n_bands, &n_rows, &n_tiles));
  *n_tiles_out = (uint32_t)n_tiles;
  const size_t n = std::min(cap_words, n_tiles * RT_TILEMASK_WORDS);
  if (n == 0) return RT_OK;
  if (!c->masks_ok) {                                        // a scene the kernels take no masks for: all ones
    for (size_t i = 0; i < n; ++i) words[i] = 0xffffffffu;
    return RT_OK;
  }
  RT_HIP(hipSetDevice(c->device));
  rt_ctx::MaskSlot* slot = nullptr;
  RT_TRY(mask_slot(c, nullptr, (int)y_first, (int)band_rows, (int)band_pitch, n_rows, n_tiles, &slot));
  RT_HIP(hipStreamSynchronize(nullptr));
  RT_HIP(hipMemcpy(words, slot->d_masks, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_scene_tile_masks(const rt_scene* s, uint32_t y_first, uint32_t band_rows, uint32_t band_pitch, uint32_t n_bands,
                        uint32_t* words, size_t cap_words, int32_t info[4]) {
  if (!s || !info || (cap_words > 0 && !words)) return fail(RT_ERR_INVALID, "null argument");
  if (s->cam_kind != RT_CAMERA_PERSPECTIVE)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_tile_masks is not built for a two-eye scene (stereoscopic / anaglyph camera)");
  rt::FlatScene f;
  RT_TRY(rt::flatten(*s, &f));
  int n_rows = 0;
  size_t n_tiles = 0;
  RT_TRY(mask_geometry(f.width, f.height, y_first, band_rows, band_pitch, n_bands, &n_rows, &n_tiles));
  RtTileMaskScene t;
  tilemask_scene(f, &t);
  info[0] = (int32_t)n_tiles;
  info[1] = t.plane;
  info[2] = (int32_t)t.boxed;
  info[3] = t.valid;
  for (size_t tile = 0; tile < n_tiles && (tile + 1) * RT_TILEMASK_WORDS <= cap_words; ++tile) {
    uint32_t* w = words + tile * RT_TILEMASK_WORDS;
    int x0, x1, y0, y1;
    if (tilemask_rect((unsigned)tile, f.width, f.height, (int)y_first, (int)band_rows, (int)band_pitch, n_rows, &x0, &x1, &y0, &y1))
      tilemask_eval(t, x0, x1, y0, y1, w);
    else
      for (int k = 0; k < RT_TILEMASK_WORDS; ++k) w[k] = 0xffffffffu;
  }
  return RT_OK;
}

}  // extern "C"
