// rt_ctx.hip -- the device context of the C ABI (include/rt_abi.h): device discovery, context
// create / free, scene upload (rt::flatten -> one HBM blob, rt_blob.h), options, own-queue streams, and what
// the row launches share: the order slots (acquire_order, finish_calibration) and finish_launch; what the side
// entries share: the host-or-device planes' Stager (their launch bracket is two lines of rt_ctx.h).
// Host code only; the kernels and their launches live in k_rows.hip, k_stereo.hip, k_wavefront.hip and the
// side entries' units (k_aa.hip, k_ortho.hip, k_assemble.hip, ...).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>

#include "rt_ctx.h"

namespace rt {

bool diag_env(const char* name) {
#ifdef RT_DIAG_ENV
  return getenv(name) != nullptr;
#else
  (void)name;
  return false;
#endif
}

void drop_order(rt_ctx::OrderSlot& s) {
  if (s.d_order) (void)hipFree(s.d_order);     // hipFree waits for work that may still read it
  if (s.d_cost) (void)hipFree(s.d_cost);
  s = rt_ctx::OrderSlot();
}
void drop_orders(rt_ctx* c) {
  for (auto& s : c->order) drop_order(s);
}
// What an order slot keeps across an upload of a scene of the same structure: the tile order, and with
// it the deferred / megakernel choice -- a deferred slot's entries carry its tiles' split (tile | part |
// log2 parts), so they are no plain permutation another kernel could take, and dropping them would make a
// host that re-uploads every frame calibrate (a host synchronisation, on the generic kernels) every
// frame.  What is reset is the one choice that is a measurement apart from the order: wavefront against
// megakernel for ray-tree scenes (wf_tune), timed again by the next ordered launch of the geometry.
void reset_order_choices(rt_ctx* c) {
  for (auto& s : c->order) s.wf_tune = 0;
}

// Tile order: reuse the measured order for this exact geometry, else calibrate on this launch.
int acquire_order(rt_ctx* c, const int32_t (&key)[8], size_t n_tiles, hipStream_t st, rt_ctx::OrderSlot** out, bool* calibrate) {
  *out = nullptr;
  *calibrate = false;
  if (!c->tile_order || n_tiles < RT_ORDER_MIN_TILES) return RT_OK;
  bool found;
  rt_ctx::OrderSlot* slot = find_slot(c->order, [&](const rt_ctx::OrderSlot& s) { return memcmp(s.key, key, sizeof key) == 0; }, &found);
  if (!found) {                       // calibrate into the empty or least recently used slot
    drop_order(*slot);
    RT_HIP(hipMalloc((void**)&slot->d_order, n_tiles * sizeof(int32_t)));
    RT_HIP(hipMalloc((void**)&slot->d_cost, n_tiles * sizeof(uint32_t)));
    RT_HIP(hipMemsetAsync(slot->d_cost, 0, n_tiles * sizeof(uint32_t), st));   // tiles that store no cost sort last
    memcpy(slot->key, key, sizeof key);
    slot->n_tiles = n_tiles;
    slot->grid = (uint32_t)n_tiles;
    slot->order_id = ++c->order_ids;
    *calibrate = true;
  }
  slot->last_use = ++c->use_clock;
  *out = slot;
  return RT_OK;
}

int finish_calibration(rt_ctx* c, hipStream_t st, rt_ctx::OrderSlot* slot, const OrderParams& p) {
  const size_t n_tiles = slot->n_tiles;
  std::vector<uint32_t> h_cost(n_tiles);
  RT_HIP(hipMemcpyAsync(h_cost.data(), slot->d_cost, n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  RT_HIP(hipStreamSynchronize(st));
  const TileOrder o = order_from_costs(h_cost, p);
  slot->masks_pay = o.masks_pay;
  slot->deferred = o.deferred;
  if (o.entries.size() > n_tiles) {   // split tiles: more entries than the calibration's table holds
    int32_t* d = nullptr;
    RT_HIP(hipMalloc((void**)&d, o.entries.size() * sizeof(int32_t)));
    (void)hipFree(slot->d_order);
    slot->d_order = d;
  }
  slot->grid = (uint32_t)o.entries.size();
  RT_HIP(hipMemcpyAsync(slot->d_order, o.entries.data(), o.entries.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  RT_HIP(hipStreamSynchronize(st));
  slot->valid = true;
  static const bool order_debug = diag_env("RT_TILE_ORDER_DEBUG");
  if (order_debug) {                  // wave times in wall-clock ticks (100 MHz)
    std::vector<uint32_t>& v = h_cost;
    std::sort(v.begin(), v.end());
    double sum = 0.0;
    for (uint32_t x : v) sum += x;
    fprintf(stderr, "tile order: %zu tiles, max %u, p99 %u, p90 %u, median %u, mean %.1f ticks; max / (sum / %.0f slots) = %.3f; "
            "ordered launches: %s kernel, %u entries\n", n_tiles, v.back(), v[n_tiles * 99 / 100], v[n_tiles * 9 / 10],
            v[n_tiles / 2], sum / n_tiles, p.slots, v.back() / (sum / p.slots), slot->deferred ? "deferred" : "mega", slot->grid);
  }
  return RT_OK;
}

int finish_launch(rt_ctx* c, hipStream_t st, const HostCopy& hc, bool mark) {
  if (c->timing) RT_HIP(hipEventRecord(c->ev1, st));
  c->timed = c->timing;
  if (mark) RT_TRY(mark_launch(c, st));
  if (hc.out) {
    RT_HIP(hipMemcpy2DAsync(hc.out, hc.stride, hc.src, hc.src_stride, hc.row_bytes, hc.n_rows, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
  }
  return RT_OK;
}

// rows between a caller's plane and its packed copy in the scratch: one copy where both are contiguous
static hipError_t copy_rows(void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t row_bytes, size_t n_rows,
                            hipMemcpyKind kind, hipStream_t st) {
  if (n_rows == 1 || (dst_stride == row_bytes && src_stride == row_bytes)) return hipMemcpyAsync(dst, src, row_bytes * n_rows, kind, st);
  return hipMemcpy2DAsync(dst, dst_stride, src, src_stride, row_bytes, n_rows, kind, st);
}

int Stager::reserve(rt_ctx* c, hipStream_t st) {
  size_t total = 0;
  for (Plane* q = pl; q < pl + n; ++q) {
    if (q->kind != TABLE) q->dev = !q->p || is_device_ptr(q->p);
    if (q->p && q->dev && q->align && (((uintptr_t)q->p | q->stride) & (q->align - 1)))
      return fail(RT_ERR_INVALID, "%s rows must be %zu-byte aligned", q->what, q->align);
    if (q->dev) continue;
    q->off = total;
    total = (total + q->row_bytes * q->n_rows + 255) & ~(size_t)255;
    staged = staged || q->kind != TABLE;
  }
  RT_TRY(ensure_scratch(c, total));
  base = (uint8_t*)c->scratch;
  for (const Plane* q = pl; q < pl + n; ++q)
    if (q->kind == IN && !q->dev)
      RT_HIP(copy_rows(base + q->off, q->row_bytes, q->p, q->stride, q->row_bytes, q->n_rows, hipMemcpyHostToDevice, st));
  return RT_OK;
}

int Stager::finish(hipStream_t st, bool must_sync) {
  for (const Plane* q = pl; q < pl + n; ++q)
    if (q->kind == OUT && !q->dev)
      RT_HIP(copy_rows(q->p, q->stride, base + q->off, q->row_bytes, q->row_bytes, q->n_rows, hipMemcpyDeviceToHost, st));
  if (staged || must_sync) RT_HIP(hipStreamSynchronize(st));
  return RT_OK;
}

int grow_device(void*& p, size_t& have, size_t need) {
  if (have >= need) return RT_OK;
  if (p) (void)hipFree(p);                  // waits for launches that may still use it
  p = nullptr;
  have = 0;
  RT_HIP(hipMalloc(&p, need));
  have = need;
  return RT_OK;
}

int ensure_scratch(rt_ctx* c, size_t bytes) { return grow_device(c->scratch, c->scratch_bytes, bytes); }

// The completion event of stream st for c (created on first use; with more than 16 streams the
// least recently added one's launches are waited for and its event reused).  Row launches BIND it to
// the kernel dispatch itself (hipExtLaunchKernel's stop event: no marker packet of its own); a
// separate hipEventRecord after every launch cost the stream 2.5-3.6 us per launch
// (profiles/r07d_marks_ab.txt: the 1080p sphere 0.0189 -> 0.0218 ms per frame).
int mark_event(rt_ctx* c, hipStream_t st, hipEvent_t* ev) {
  for (auto& m : c->marks)
    if (m.s == st) {
      *ev = m.ev;
      return RT_OK;
    }
  rt_ctx::Mark m{st, nullptr};
  if (c->marks.size() >= 16) {
    m.ev = c->marks.front().ev;
    RT_HIP(hipEventSynchronize(m.ev));
    c->marks.erase(c->marks.begin());
  } else {
    RT_HIP(hipEventCreateWithFlags(&m.ev, hipEventDisableTiming));
  }
  c->marks.push_back(m);
  *ev = m.ev;
  return RT_OK;
}

int mark_launch(rt_ctx* c, hipStream_t st) {
#ifdef RT_DIAG_NO_MARKS
  return RT_OK;                       // diagnostic builds only: the marks' cost (A/B)
#endif
  hipEvent_t ev = nullptr;
  RT_TRY(mark_event(c, st, &ev));
  RT_HIP(hipEventRecord(ev, st));
  return RT_OK;
}

int wait_launches(rt_ctx* c) {
  for (auto& m : c->marks) RT_HIP(hipEventSynchronize(m.ev));
  return RT_OK;
}

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace rt

using rt::drop_orders;

template <typename T>
static size_t put(std::vector<uint8_t>& blob, const std::vector<T>& v) {
  size_t off = (blob.size() + 255) & ~(size_t)255;
  blob.resize(off + v.size() * sizeof(T) + 16);
  if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
  return off;
}

extern "C" {

int rt_device_count(int* count) {
  if (!count) return fail(RT_ERR_INVALID, "null output");
  *count = 0;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) { *count = 0; return fail(RT_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  return RT_OK;
}

int rt_ctx_create(int device, rt_ctx** out) {
  if (!out) return fail(RT_ERR_INVALID, "null output");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_DEVICE, "no HIP device available");
  if (device < 0 || device >= n) return fail(RT_ERR_INVALID, "device %d out of range (%d devices)", device, n);
  RT_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  RT_HIP(hipGetDeviceProperties(&prop, device));
  rt_ctx* c = new rt_ctx();
  c->device = device;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  memset(&c->dev, 0, sizeof c->dev);
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->tev0) != hipSuccess || hipEventCreate(&c->tev1) != hipSuccess) {
    delete c;
    return fail(RT_ERR_DEVICE, "stream/event creation failed");
  }
  *out = c;
  return RT_OK;
}

int rt_ctx_upload(rt_ctx* c, const rt_scene* s) {
  if (!c || !s) return fail(RT_ERR_INVALID, "null argument");
  rt::FlatScene f;
  int rc = rt::flatten(*s, &f);
  if (rc) return rc;
  std::vector<uint8_t> blob;
  size_t o_obj = put(blob, f.objects), o_trav = put(blob, f.trav), o_strav = put(blob, f.strav), o_nodes = put(blob, f.nodes),
         o_leaves = put(blob, f.leaves);
  std::vector<RtTravC> travc, stravc;
  for (const auto* src : {&f.trav, &f.strav}) {
    std::vector<RtTravC>& dst = src == &f.trav ? travc : stravc;
    dst.resize(src->size());
    for (size_t i = 0; i < src->size(); ++i) {
      const RtTrav& t = (*src)[i];
      if ((uint32_t)t.skip >= (1u << 28)) return fail(RT_ERR_UNSUPPORTED, "object hierarchy of more than 2^28 nodes");
      for (int k = 0; k < 3; ++k) { dst[i].lo[k] = t.fblo[k]; dst[i].hi[k] = t.fbhi[k]; }
      dst[i].obj = t.obj;
      dst[i].skip_flags = (uint32_t)t.skip | (uint32_t)t.cull << 28 | (uint32_t)(t.shadow_skip ? 1 : 0) << 30;
    }
  }
  const size_t o_travc = put(blob, travc), o_stravc = put(blob, stravc);
  size_t o_prog = put(blob, f.prog), o_lights = put(blob, f.lights), o_tex = put(blob, f.textures);
  size_t o_texels = put(blob, f.texels);
  // camera_ray's terms of the integer pixels (rt_device.h camera_ray_px): the same expressions in the
  // same order, IEEE double on the host (-ffp-contract=off as the device), so a table entry is the
  // value the device would compute
  std::vector<double> csx((size_t)std::max(0, f.width)), csy((size_t)std::max(0, f.height));
  for (size_t x = 0; x < csx.size(); ++x) csx[x] = (((double)x / f.cam.width) - 0.5) * f.cam.aspect;
  for (size_t y = 0; y < csy.size(); ++y) csy[y] = (f.cam.height - 1.0 - (double)y) / f.cam.height - 0.5;
  size_t o_csx = put(blob, csx), o_csy = put(blob, csy);
  // Two-eye scenes (rt_blob.h RtViews): each view's column table, the same expressions with the eye
  // camera's width and aspect ratio.  Stereoscopic (camera.rs:124-128): the RIGHT eye fills columns
  // [0, w), w = W / 2, the left eye [w, W) at x - w -- for odd W its last column is x - w = w, one past
  // the eye cameras' nominal width, which create_ray defines all the same.  Anaglyph (:186-195): both
  // eyes cover the frame, the left stores R, the right G, B and A.
  RtViews views = {};
  size_t o_vsx[2] = {0, 0};
  if (f.cam_kind != RT_CAMERA_PERSPECTIVE) {
    const bool stereo = f.cam_kind == RT_CAMERA_STEREOSCOPIC;
    const int32_t w = f.width / 2;
    views.kind = f.cam_kind;
    views.stereo_w = w;
    for (int i = 0; i < 2; ++i) {
      RtView& v = views.v[i];
      v.cam = stereo ? f.eye[1 - i] : f.eye[i];
      v.x0 = stereo && i == 1 ? w : 0;
      v.width = !stereo ? f.width : i == 0 ? w : f.width - w;
      v.tiles_x = (v.width + RT_TILE_W - 1) / RT_TILE_W;
      v.channels = stereo ? RT_VIEW_RGBA : i == 0 ? RT_VIEW_R : RT_VIEW_GBA;
      std::vector<double> vsx((size_t)std::max(0, v.width));
      for (size_t x = 0; x < vsx.size(); ++x) vsx[x] = (((double)x / v.cam.width) - 0.5) * v.cam.aspect;
      o_vsx[i] = put(blob, vsx);
    }
  }
  bool masks_ok = false;
  const size_t o_mask = rt::put_mask_scene(f, blob, &masks_ok);
  RT_HIP(hipSetDevice(c->device));
  RT_TRY(rt::wait_launches(c));       // launches in flight read the blob and may run the specialised modules
  rt::drop_masks(c);                  // the masks depend on the camera and on every position: never kept
  if (c->d_blob) { (void)hipFree(c->d_blob); c->d_blob = nullptr; }
  c->uploaded = false;
  RT_HIP(hipMalloc(&c->d_blob, blob.size()));
  RT_HIP(hipMemcpy(c->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  c->blob_bytes = blob.size();
  uint8_t* b = (uint8_t*)c->d_blob;
  RtDevScene& d = c->dev;
  d.objects = (const RtObject*)(b + o_obj);
  d.trav = (const RtTrav*)(b + o_trav);
  d.n_trav = (int32_t)f.trav.size();
  d.strav = (const RtTrav*)(b + o_strav);
  d.trav_c = (const RtTravC*)(b + o_travc);
  d.strav_c = (const RtTravC*)(b + o_stravc);
  d.n_strav = (int32_t)f.strav.size();
  d.nodes = (const RtNode*)(b + o_nodes);
  d.leaves = (const RtLeaf*)(b + o_leaves);
  d.prog = (const RtProg*)(b + o_prog);
  d.lights = (const RtLight*)(b + o_lights);
  d.textures = (const RtTexture*)(b + o_tex);
  d.texels = b + o_texels;
  d.cam_sx = (const double*)(b + o_csx);
  d.cam_sy = (const double*)(b + o_csy);
  c->d_mask_scene = b + o_mask;
  c->masks_ok = masks_ok;
  c->sky_ok = rt::tilemask_sky_ok(f);
  c->mask_plane = rt::tilemask_plane(f);
  c->last_sky_slot = nullptr;
  c->last_lean_slot = nullptr;
  c->last_rec_slot = nullptr;
  c->last_traced = false;
  c->launches_since_upload = 0;
  d.n_objects = (int32_t)f.objects.size();
  d.n_lights = (int32_t)f.lights.size();
  d.n_leaves = (int32_t)f.leaves.size();
  d.n_nodes = (int32_t)f.nodes.size();
  d.width = f.width;
  d.height = f.height;
  d.any_transparent = f.any_transparent;
  d.shadow_early_out = f.shadow_early_out;
  d.colour_fast = f.colour_fast;
  d.ray_chains = f.ray_chains;
  d.shadow_pow = f.shadow_pow;
  d.shadow_t = f.shadow_t;
  d.cam = f.cam;
  const int32_t prev_kind = c->views.kind;
  c->views = views;
  for (int i = 0; i < 2 && views.kind; ++i) c->views.v[i].cam_sx = (const double*)(b + o_vsx[i]);
  c->max_depth = f.max_depth;
  {                                   // the wavefront path's key extent: the hull of the bounded objects
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const RtObject& o : f.objects)
      if (o.cull == RT_CULL_BOX)
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], o.blo[k]); hi[k] = std::max(hi[k], o.bhi[k]); }
    for (int k = 0; k < 3; ++k) {
      const bool ok = std::isfinite(lo[k]) && std::isfinite(hi[k]) && hi[k] > lo[k];
      c->wf_klo[k] = ok ? lo[k] : f.cam.center[k] - 100.0;
      c->wf_khi[k] = ok ? hi[k] : f.cam.center[k] + 100.0;
    }
  }
  c->uploaded = true;
  // Tile costs belong to the previous scene -- unless the new one has its structure (the same scene
  // rebuilt, or the next frame of an animation: a host shaped like the reference's GUI rebuilds and
  // uploads the scene every frame, debug_window.rs:53-68, gui.rs:78-89).  Then its orders stay: any
  // tile order renders the same pixels, the old one is near the new costs, and the first launch after
  // the upload takes an ordered (non-calibrating) kernel -- the specialised one, whose programs have no
  // calibration variant at the default level (a calibrating launch would run the generic kernels).
  // The ray-tree scenes' wavefront / megakernel choice is measured again (reset_order_choices); the tile
  // masks, which depend on the camera and on every position, were dropped above whatever the structure.
  // The camera kind counts as structure here: a two-eye launch has other tiles (two views') and other
  // kernels, and an upload of a perspective scene after a two-eye one behaves as on a fresh context.
  if (!(c->spec.flat && prev_kind == f.cam_kind && rt::same_structure_flat(*c->spec.flat, f))) drop_orders(c);
  else rt::reset_order_choices(c);
  // the scene-specialised programs (spec_ctx.hip): requested from the compile pool, loaded by the first
  // launch after they are ready; the generic kernels render until then.  Only the flags are computed
  // here -- the program text (and a family lookup) only when the option is on and the scene fits.
  rt::spec_drop(c);                   // the previous scene's modules (the hipFree above waited for the device)
  c->spec.flat = std::make_shared<rt::FlatScene>(std::move(f));
  c->spec.flat->texels.clear();
  c->spec.flat->texels.shrink_to_fit();
  rt::spec_prepare(c);
  return RT_OK;
}

int rt_ctx_kernel_info(rt_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap == 0) return fail(RT_ERR_INVALID, "null argument");
  std::string s;
  char b[1024];
  const rt_ctx::Spec& S = c->spec;
  if (S.loaded) {
    snprintf(b, sizeof b, "scene-specialised (hipRTC %016llx, %s%s, compiled in %.0f ms%s by %s; %s; loaded %.0f ms after "
             "the request)", (unsigned long long)S.hash,
             S.prog.mode == RT_MODE_REFL ? "reflection" : S.prog.mode == RT_MODE_CHAIN ? "chain" : "tree",
             S.prog.family ? (", family of " + std::to_string(S.prog.family) + " scenes").c_str() : "",
             S.compile_ms, S.note.c_str(), rt::spec_compiler().origin.c_str(), S.res.c_str(), S.ready_ms);
    s = b;
  } else if (S.level && c->uploaded && !S.prog.fits) {
    snprintf(b, sizeof b, "generic (librt_mi355x.so; scene too large to specialise: > %d objects or > %d leaves)",
             RT_SPEC_MAX_OBJECTS, RT_SPEC_MAX_LEAVES);
    s = b;
  } else if (S.level && c->uploaded && S.pending) {
    s = "generic (librt_mi355x.so; the scene-specialised program is compiling in the background)";
  } else if (S.level && c->uploaded && !S.error.empty()) {
    s = "generic (librt_mi355x.so; specialisation failed: " + S.error + ")";
  } else {
    s = "generic (librt_mi355x.so)";
  }
  // sky fill: the last launch's records could say sky; the counts come from a pinned word once the records'
  // gather has completed (no wait: "counts pending" until then, no counts once the table has been dropped).
  // (Ahead of "last launch": callers match the text from there to the end.)
  // traced masks: the last launch's record table went through the trace pass (ahead of "lean tiles": callers
  // match "; lean tiles: ...; sky fill: ...; last launch:" as one run of text)
  s += c->last_traced ? "; traced masks: on" : "; traced masks: off";
  const int64_t n_lean = c->last_lean_slot ? rt::record_lean_entries(c, c->last_lean_slot, c->last_lean_id) : -1;
  s += !c->last_lean_slot ? "; lean tiles: off" + (c->lean_tiles ? rt::spec_lean_note(c) : std::string())
       : n_lean >= 0      ? "; lean tiles: on (" + std::to_string(n_lean) + " entries)"
       : n_lean == -2     ? "; lean tiles: on (count pending)"
                          : "; lean tiles: on";
  uint32_t n_entries = 0;
  const int64_t n_sky = c->last_sky_slot ? rt::record_sky_entries(c, c->last_sky_slot, c->last_sky_id, &n_entries) : -1;
  if (n_sky >= 0)
    s += "; sky fill: on (" + std::to_string((int64_t)n_entries - n_sky) + " render, " + std::to_string(n_sky) + " sky entries)";
  else
    s += !c->last_sky_slot ? "; sky fill: off" : n_sky == -2 ? "; sky fill: on (counts pending)" : "; sky fill: on";
  s += std::string("; last launch: ") + c->last_kernel;
  s += c->last_masked ? "; tile masks: on" : "; tile masks: off";
  s += c->last_records ? "; tile records: on" : "; tile records: off";
  snprintf(buf, cap, "%s", s.c_str());
  return RT_OK;
}

int rt_ctx_spec_wait(rt_ctx* c, int32_t timeout_ms) {
  if (!c) return fail(RT_ERR_INVALID, "null context");
  RT_HIP(hipSetDevice(c->device));
  const int rc = rt::spec_wait(c, (double)timeout_ms);
  if (rc == RT_PENDING) return RT_PENDING;
  if (!c->spec.error.empty()) return fail(RT_ERR_UNSUPPORTED, "%s", c->spec.error.c_str());
  return RT_OK;
}

int rt_ctx_spec_wait_samples(rt_ctx* c, int32_t timeout_ms) {
  if (!c) return fail(RT_ERR_INVALID, "null context");
  RT_HIP(hipSetDevice(c->device));
  if (rt::spec_samples_wait(c, (double)timeout_ms) == RT_PENDING) return RT_PENDING;
  for (int kind = 0; kind < rt::SPEC_KINDS; ++kind)
    if (rt::spec_is_sample(kind) && !c->spec.slots[kind][0][0].error.empty())
      return fail(RT_ERR_UNSUPPORTED, "%s: %s", rt::spec_kind(kind).name, c->spec.slots[kind][0][0].error.c_str());
  return RT_OK;
}

int rt_ctx_sample_kernel_info(rt_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap == 0) return fail(RT_ERR_INVALID, "null argument");
  snprintf(buf, cap, "%s", rt::spec_sample_info(c).c_str());
  return RT_OK;
}

int rt_ctx_last_kernel_ms(rt_ctx* c, float* ms) {
  if (!c || !ms) return fail(RT_ERR_INVALID, "null argument");
  if (!c->timed) return fail(RT_ERR_INVALID, c->timing ? "no launch recorded" : "RT_OPT_TIMING is off");
  RT_HIP(hipEventSynchronize(c->ev1));
  RT_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return RT_OK;
}

int rt_ctx_set_option(rt_ctx* c, int32_t option, int32_t value) {
  if (!c) return fail(RT_ERR_INVALID, "null context");
  if (option == RT_OPT_TIMING) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "RT_OPT_TIMING value %d", value);
    c->timing = value != 0;
    c->timed = false;                  // no launch recorded under the new setting yet
    return RT_OK;
  }
  if (option == RT_OPT_SPECIALIZE) {
    if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "RT_OPT_SPECIALIZE value %d", value);
    const bool retry = value == c->spec.level && !c->spec.error.empty();   // the same value again: compile again
    if (value == c->spec.level && !retry) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    int rc = rt::wait_launches(c);              // this context's launches in flight may still run the modules
    if (rc) return rc;
    rt::spec_drop(c);
    c->spec.level = value;
    if (c->uploaded) rt::spec_prepare(c, retry);   // a scene family registered since the upload may hold it
    return RT_OK;
  }
  if (option == RT_OPT_SPEC_SAMPLES) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "RT_OPT_SPEC_SAMPLES value %d", value);
    c->spec.samples = value;                  // loaded kernels stay: the points / AA calls just stop (or start) taking them
    return RT_OK;
  }
  if (option == RT_OPT_TILE_MASKS) {
    if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "RT_OPT_TILE_MASKS value %d", value);
    c->tile_masks = value;               // the tables stay: launches just stop (or start) passing them
    return RT_OK;
  }
  if (option == RT_OPT_TILE_RECORDS) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "RT_OPT_TILE_RECORDS value %d", value);
    c->tile_records = value != 0;        // the tables stay: launches just stop (or start) passing them
    return RT_OK;
  }
  if (option == RT_OPT_SKY_FILL) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "RT_OPT_SKY_FILL value %d", value);
    c->sky_fill = value != 0;            // record tables are keyed by it: the next launch gathers its own
    return RT_OK;
  }
  if (option == RT_OPT_LEAN_TILES) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "RT_OPT_LEAN_TILES value %d", value);
    c->lean_tiles = value != 0;          // record tables are keyed by it: the next launch gathers its own
    return RT_OK;
  }
  if (option == RT_OPT_TRACED_MASKS) {
    if (value < 0 || value > 3) return fail(RT_ERR_INVALID, "RT_OPT_TRACED_MASKS value %d", value);
    c->traced_masks = value;             // record tables are keyed by what a launch takes: the next one gathers its own
    return RT_OK;
  }
  if (option == RT_OPT_WAVEFRONT_PAIRS) {
    if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "RT_OPT_WAVEFRONT_PAIRS %d not in [0, 2]", value);
    c->wf_pairs = value;
    return RT_OK;
  }
  if (option == RT_OPT_WAVEFRONT_CAP) {
    if (value < 1 || value > 400) return fail(RT_ERR_INVALID, "RT_OPT_WAVEFRONT_CAP %d not in [1, 400]", value);
    c->wf_cap_pct = value;
    return RT_OK;
  }
  if (option == RT_OPT_TILE_ORDER || option == RT_OPT_FAST_CLAMP) {
    if (value != 0 && value != 1) return fail(RT_ERR_INVALID, "option %d value %d", option, value);
    if (option == RT_OPT_FAST_CLAMP) {
      c->fast_clamp = value != 0;
    } else if (c->tile_order != (value != 0)) {
      RT_HIP(hipSetDevice(c->device));
      drop_orders(c);
      c->tile_order = value != 0;
    }
    return RT_OK;
  }
  if (option != RT_OPT_KERNEL) return fail(RT_ERR_INVALID, "unknown option %d", option);
  if (value != RT_KERNEL_AUTO && value != RT_KERNEL_MEGA && value != RT_KERNEL_DEFERRED && value != RT_KERNEL_WAVEFRONT)
    return fail(RT_ERR_INVALID, "RT_OPT_KERNEL value %d", value);
  if (value != c->kernel_opt) {
    // tile orders were built for one kernel (split entries only for the deferred one): rebuild
    RT_HIP(hipSetDevice(c->device));
    drop_orders(c);
    c->kernel_opt = value;
  }
  return RT_OK;
}

int rt_stream_create(int device, void** stream) {
  if (!stream) return fail(RT_ERR_INVALID, "null argument");
  int n_dev = 0;
  RT_HIP(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(RT_ERR_INVALID, "device %d of %d", device, n_dev);
  RT_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  RT_HIP(hipGetDeviceProperties(&prop, device));
  // every CU enabled: the mask only buys the stream a hardware queue of its own
  std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, 0xFFFFFFFFu);
  if (prop.multiProcessorCount % 32) mask.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
  hipStream_t st = nullptr;
  RT_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  *stream = st;
  return RT_OK;
}

int rt_stream_destroy(void* stream) {
  if (!stream) return fail(RT_ERR_INVALID, "null stream");
  RT_HIP(hipStreamDestroy((hipStream_t)stream));
  return RT_OK;
}

int rt_ctx_synchronize(rt_ctx* c) {
  if (!c) return fail(RT_ERR_INVALID, "null context");
  RT_HIP(hipSetDevice(c->device));
  return rt::wait_launches(c);
}

void rt_ctx_free(rt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // this context's own launches, through its completion events: not the device (other contexts'
  // work), not a caller's stream (bench.py's frames-in-flight streams are destroyed by now;
  // synchronising a destroyed stream crashed at exit in round 4)
  (void)rt::wait_launches(c);
  for (auto& m : c->marks) (void)hipEventDestroy(m.ev);
  c->marks.clear();
  if (c->d_blob) (void)hipFree(c->d_blob);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->wf) (void)hipFree(c->wf);
  if (c->wfr) (void)hipFree(c->wfr);
  if (c->wfp) (void)hipFree(c->wfp);
  drop_orders(c);
  rt::drop_masks(c);
  rt::spec_drop(c);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->tev0) (void)hipEventDestroy(c->tev0);
  if (c->tev1) (void)hipEventDestroy(c->tev1);
  delete c;
}

}  // extern "C"
