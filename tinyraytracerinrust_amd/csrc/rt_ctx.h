// rt_ctx.h -- the device context behind the C ABI (include/rt_abi.h: rt_ctx_*), shared by the
// host halves of the kernel translation units: rt_ctx.hip (create / upload / options / streams),
// k_rows.hip (the row kernels' launches), k_stereo.hip (two-eye scenes' launches), k_masks.hip (tile masks and
// dispatch records), k_wavefront.hip (the wavefront path's level kernels and its launch), k_wf_pairs.hip (its pair
// path), the side entries' units (k_aa.hip, k_ortho.hip, k_assemble.hip, k_points.hip, k_stats.hip, k_hits.hip,
// k_paths.hip), spec_ctx.hip.  The launches' decisions are launch_plan.h's and wf_plan.h's (pure host code,
// no HIP); this header holds what they share on the device side: the slot cache, the order
// slots' acquisition and calibration, the end of a launch, the side entries' bracket and plane stager, the
// template dispatch.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "launch_plan.h"
#include "wf_plan.h"
#include "rt_blob.h"
#include "scene.h"
#include "spec.h"


struct rt_ctx {
  int device = 0;
  void* d_blob = nullptr;
  size_t blob_bytes = 0;
  RtDevScene dev;
  RtViews views = {};                   // two-eye scenes (views.kind != 0): the two views' cameras and column tables
  int32_t max_depth = 10;
  int32_t kernel_opt = RT_KERNEL_AUTO;  // rt_ctx_set_option(RT_OPT_KERNEL)
  bool timing = true;                   // rt_ctx_set_option(RT_OPT_TIMING): launch events recorded
  bool tile_order = true;               // rt_ctx_set_option(RT_OPT_TILE_ORDER): cost-ordered dispatch
  bool fast_clamp = true;               // rt_ctx_set_option(RT_OPT_FAST_CLAMP): min/max clamps where exact
  int wf_cap_pct = 200;                 // rt_ctx_set_option(RT_OPT_WAVEFRONT_CAP): rays per level, % of pixel slots
  double wf_klo[3] = {-100, -100, -100}, wf_khi[3] = {100, 100, 100};   // coherence-key extent (bounded objects)
  int n_cu = 256;                       // compute units of the device (wave slots = n_cu x 4 SIMDs x waves/SIMD)
  bool uploaded = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t tev0 = nullptr, tev1 = nullptr;   // the wavefront autotune's own pair
  bool timed = false;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* wf = nullptr;                   // wavefront arena (levels, counters, overflow flags), grow-only
  size_t wf_bytes = 0;
  int wf_pairs = 1;                     // rt_ctx_set_option(RT_OPT_WAVEFRONT_PAIRS): 0 off, 1 levels >= 1, 2 every level
  int wfp_occ[2] = {0, 0};              // candidate kernels (nearest, shadow): workgroups per CU at wfp_occ_lds bytes of LDS
  size_t wfp_occ_lds[2] = {0, 0};
  void* wfr = nullptr;                  // pair path: per-ray arrays (nearest hit, hit point, shadow counts), grow-only
  size_t wfr_bytes = 0;
  void* wfp = nullptr;                  // pair path: pair lists + sort scratch, grow-only
  size_t wfp_bytes = 0;
  uint32_t wfp_cap = 0;
  // Cost-ordered tile dispatch.  A frame's time is set by its slowest tiles (long reflection
  // chains), so they are dispatched first: the first launch of a geometry records every tile's
  // wave time, and later launches of the same geometry read the tiles in descending cost order.
  // One table per geometry key (rows, bands, depth, f64, width), RT_ORDER_SLOTS of them, LRU.
  // A table is written exactly once (its calibration, synchronous) and never rewritten while it
  // exists, so launches queued on other streams can never read a half-written order; tables are
  // freed only by hipFree (which waits for the device) on eviction, upload or rt_ctx_free.
  struct OrderSlot {
    int32_t key[8] = {0};             // y_first, band_rows, band_pitch, n_rows, depth, f64, width, camera kind
    int32_t* d_order = nullptr;
    uint32_t* d_cost = nullptr;
    size_t n_tiles = 0;
    uint32_t grid = 0;                // entries of the order (> n_tiles when costly tiles are split)
    uint64_t last_use = 0;
    bool deferred = false;            // ordered launches take the deferred-shadow kernel
    int wf_tune = 0;                  // ray-tree scenes, RT_KERNEL_AUTO: 0 not yet timed, 1 megakernel, 2 wavefront
    bool masks_pay = false;           // the calibration found the launch throughput-bound: the masked megakernel
                                      // (RT_OPT_TILE_MASKS 1); kept with the order across same-structure uploads
    bool valid = false;               // set once the sorted order is on the device
    uint64_t order_id = 0;            // which calibration of the context wrote d_order (RecSlot; never 0)
  };
  static constexpr int RT_ORDER_SLOTS = 8;
  OrderSlot order[RT_ORDER_SLOTS];
  uint64_t use_clock = 0;
  // Per-tile object masks (rt_tilemask.h, k_masks.hip): one table of RT_TILEMASK_WORDS words per tile
  // and launch geometry (rows, bands, width: the masks depend on neither depth nor output format, and
  // launches too small for a tile order take them as well, so the tables have slots of their own
  // beside the orders').  Unlike a tile order a table depends on the camera and on every object's
  // position: it is DROPPED ON EVERY UPLOAD and filled again by the first launch of its geometry after
  // it -- one small kernel on that launch's stream ahead of the render, no host synchronisation.
  // `ready` is recorded after the fill; launches on other streams wait for it on the device until the
  // host has seen it complete.
  struct MaskSlot {
    int32_t key[5] = {0};             // y_first, band_rows, band_pitch, n_rows, width
    uint32_t* d_masks = nullptr;
    size_t n_tiles = 0;
    uint64_t last_use = 0;
    hipStream_t fill_stream = nullptr;
    hipEvent_t ready = nullptr;
    uint64_t fill_id = 0;             // which fill of the context this table is (RecSlot)
    bool seen_ready = false;
    bool valid = false;
  };
  static constexpr int RT_MASK_SLOTS = 8;
  MaskSlot masks[RT_MASK_SLOTS];
  // Dispatch records (rt_blob.h RtTileRec, k_masks.hip): per order entry of a masked launch the tile's first
  // column, first output row and mask words, gathered on the device from the geometry's mask table and the
  // launch's tile order (null: the identity) -- one scalar load in the kernel where the order, the tile
  // division and the mask words were dependent trips.  A table is keyed by its two inputs, each named by a
  // number the context never reuses: the mask fill it read (MaskSlot::fill_id -- masks are dropped on every
  // upload and filled again) and the calibration that wrote its order (OrderSlot::order_id, 0: no order).  A
  // table of an earlier fill or order is therefore never found again; its successor is gathered on the
  // launch's stream, behind the mask fill, with no host synchronisation.  Launches on other streams wait for
  // `ready` as they do for the masks'.  Same LRU and free rules as the mask tables.
  struct RecSlot {
    uint64_t order_id = 0;            // the order gathered from (0: the identity)
    uint64_t fill_id = 0;             // the mask fill gathered from
    RtTileRec* d_recs = nullptr;
    uint32_t* d_sky = nullptr;        // behind the table: how many records say sky, copied on the gather's stream
    uint32_t* h_sky = nullptr;        //   to this pinned host word ahead of `ready` (rt_ctx_kernel_info reads it
    uint64_t rec_id = 0;              //   once hipEventQuery says so, never waiting); rec_id: never reused
    bool sky_fill = false;            // gathered with RT_OPT_SKY_FILL on for a scene that can have sky tiles
    bool lean = false;                // gathered with the lean bits and checked (RT_OPT_LEAN_TILES); the entries that
                                      //   kept theirs follow the sky count: d_sky / h_sky [1] their number, [2] ~first
                                      //   entry, [3] last entry + 1 (both 0: none)
    int traced = 0;                   // its words and lean bits are the trace pass's (RT_OPT_TRACED_MASKS): 1 the
                                      //   floor-only entries', 2 the entries with an object pixel too (r0's flag)
    uint32_t n_entries = 0;           // order entries = records
    uint64_t last_use = 0;
    hipStream_t fill_stream = nullptr;
    hipEvent_t ready = nullptr;
    bool seen_ready = false;
    bool valid = false;
  };
  static constexpr int RT_REC_SLOTS = 8;
  RecSlot recs[RT_REC_SLOTS];
  uint64_t mask_fills = 0, order_ids = 0;   // count mask fills and calibrations: MaskSlot::fill_id, OrderSlot::order_id
  bool tile_records = true;             // rt_ctx_set_option(RT_OPT_TILE_RECORDS)
  bool last_records = false;            // the last row launch passed a record table (rt_ctx_kernel_info)
  // Sky tiles (rt_ctx_set_option(RT_OPT_SKY_FILL), rt_device.h rows_entry): a record whose prim word is 0
  // makes its wave store BLACK and return.  sky_ok, mask_plane: the uploaded scene's (k_masks.hip
  // tilemask_sky_ok, tilemask_plane); last_sky_*: the last row launch's record table, where it can say sky.
  bool sky_fill = true;
  bool sky_ok = false;
  int mask_plane = -1;
  const void* last_sky_slot = nullptr;
  uint64_t last_sky_id = 0, rec_ids = 0;
  // Lean tiles (rt_ctx_set_option(RT_OPT_LEAN_TILES), rt_bodies.h lean_body): the entries whose record carries
  // the lean bit are rendered by the program's lean kernel ahead of the megakernel.  last_lean_*: the last row
  // launch's record table where it took the lean kernel.
  bool lean_tiles = true;
  const void* last_lean_slot = nullptr;
  uint64_t last_lean_id = 0;
  // Traced tile masks (rt_ctx_set_option(RT_OPT_TRACED_MASKS), rt_bodies.h trace_masks_body): 0 never, 1 where the
  // masked megakernel runs by the library's own choice (LaunchPlan::traced), 2 / 3 every megakernel launch with records;
  // 2 takes the floor-only form of table, 1 and 3 the form whose object entries are traced too (LaunchPlan::traced_objects).
  // last_traced: the last row launch's table was traced; last_rec_*: that table, whatever it holds
  // (rt_ctx_tile_records).
  int traced_masks = 1;
  uint32_t launches_since_upload = 0;   // row launches since rt_ctx_upload (value 1 waits for RT_TRACED_MIN_LAUNCHES)
  bool last_traced = false;
  const void* last_rec_slot = nullptr;
  uint64_t last_rec_id = 0;
  int tile_masks = 1;                  // rt_ctx_set_option(RT_OPT_TILE_MASKS): 0 never, 1 where they pay (OrderSlot::masks_pay), 2 always
  bool masks_ok = false;                // the uploaded scene has a mask scene in its blob (<= 32 objects)
  const void* d_mask_scene = nullptr;   // RtTileMaskScene in the blob
  bool last_masked = false;             // the last row launch passed a mask table (rt_ctx_kernel_info)
  // Scene-specialised kernels (spec.h, rt_ctx_set_option(RT_OPT_SPECIALIZE)): hipRTC compiles rt_device.h
  // with this scene's tables as constexpr data, in the background (the library's compile pool); launches
  // take them once they are loaded (spec_poll), the generic kernels until then.
  // One slot per kernel of the catalogue, (kind, f64, cal).  The row kinds are one job set, loaded all or
  // nothing (`loaded`; a failure drops them and sets `error`).  The sample kinds (rt_render_points_f64 and
  // rt_antialias' trace passes, RT_OPT_SPEC_SAMPLES) are a second: requested by the first such call after an
  // upload (and by every later upload once a context has asked), behind the row programs in the pool; each
  // loads, fails and is reported on its own, and nothing of theirs touches the row programs' state.
  struct SpecSlot {
    std::shared_ptr<rt::SpecJob> job;   // requested, not yet loaded
    hipModule_t module = nullptr;       // on this context's device
    hipFunction_t function = nullptr;   // non-null once loaded (null: the generic kernel)
    std::string error;                  // a sample path: why it stays generic although requested
    std::string res;                    // the loaded kernel's resources (a sample kernel's: compile time and provenance too)
    bool cached = false;                // the code object existed in the process when it was requested
  };
  struct Spec {
    int level = 1;                      // RT_OPT_SPECIALIZE: 0 off, 1 (default) product launches, 2 every row launch
    int samples = 1;                    // RT_OPT_SPEC_SAMPLES
    rt::SpecProgram prog;               // the uploaded scene's program (spec_describe)
    std::shared_ptr<rt::FlatScene> flat;   // the uploaded scene's tables (texels dropped): the program is
                                        // chosen when the option is set (families registered since the upload)
    SpecSlot slots[rt::SPEC_KINDS][2][2];   // [kind][f64][cal]
    bool pending = false;               // row programs requested, not yet loaded
    bool loaded = false;                // the row kernels are loaded (false: generic kernels)
    std::string error;                  // why the context keeps the generic kernels although `level` (kernel info)
    std::string note;                   // " [process cache]" / " [disk cache]"
    std::string res;                    // the loaded megakernel's resources (kernel info)
    uint64_t hash = 0;                  // FNV-1a of the prelude (kernel info only; caches compare full texts)
    double compile_ms = 0.0;            // the hipRTC time of the loaded programs (0: read from the disk cache)
    double t0 = 0.0;                    // when the programs were requested (steady clock, ms)
    double ready_ms = 0.0;              // request -> loaded, ms
    bool samples_wanted = false;        // a points / AA call (or rt_ctx_spec_wait_samples) has asked: uploads request them
    const char* last_sample = "none";   // what the last points / AA trace launch ran (rt_ctx_sample_kernel_info)
  } spec;
  // Completion marks: per stream this context launched on, an event recorded after its last launch
  // there.  rt_ctx_synchronize / option changes / rt_ctx_free wait on them -- never on a caller's
  // stream, which may be destroyed by then.
  struct Mark { hipStream_t s; hipEvent_t ev; };
  std::vector<Mark> marks;
  const char* last_kernel = "none";     // what the last row launch ran (rt_ctx_kernel_info)
};

using rt::fail;

#define RT_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

namespace rt {
// The slot cache of the order, mask and record tables: the valid slot that `match` accepts (*found), else the
// slot to fill -- an empty one, or the least recently used.  The caller drops and fills it: those differ.
template <class Slot, size_t N, class Match>
Slot* find_slot(Slot (&slots)[N], Match match, bool* found) {
  Slot* lru = &slots[0];
  *found = true;
  for (auto& s : slots)
    if (s.valid && match(s)) return &s;
  *found = false;
  for (auto& s : slots) {
    if (!s.valid) return &s;
    if (s.last_use < lru->last_use) lru = &s;
  }
  return lru;
}
// A launch on st reads a table (MaskSlot, RecSlot) filled on another stream: after the fill, on the device,
// until the host has seen the fill complete.
template <class Slot>
int wait_ready(Slot& s, hipStream_t st) {
  if (s.seen_ready || s.fill_stream == st) return RT_OK;
  if (hipEventQuery(s.ready) == hipSuccess) {
    s.seen_ready = true;
    return RT_OK;
  }
  (void)hipGetLastError();
  RT_HIP(hipStreamWaitEvent(st, s.ready, 0));
  return RT_OK;
}
// Runtime flags to template arguments: f(std::bool_constant / std::integral_constant values...).  The generic
// row, deferred and view kernels are instantiated through these, each combination once.
template <class F>
void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
void with_mode(int mode, F&& f) {
  if (mode == RT_MODE_CHAIN) f(std::integral_constant<int, RT_MODE_CHAIN>{});
  else if (mode == RT_MODE_TREE) f(std::integral_constant<int, RT_MODE_TREE>{});
  else f(std::integral_constant<int, RT_MODE_REFL>{});
}
template <class F>
void with_span(int span, F&& f) {   // the wavefront fold's levels per launch: 1, 2 or 3
  if (span >= 3) f(std::integral_constant<int, 3>{});
  else if (span == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}
template <class F>
void with_flags(bool f64, bool cal, bool fc, F&& f) {   // f(F64, CAL, FC)
  with_bool(f64, [&](auto d) { with_bool(cal, [&](auto c) { with_bool(fc, [&](auto k) { f(d, c, k); }); }); });
}
// rt_ctx.hip
// The order slot of a launch of n_tiles tiles with geometry `key` on st: null below RT_ORDER_MIN_TILES or with
// the tile order off; *calibrate: the slot is new (its tables allocated, the costs zeroed on st) and this
// launch measures it.  finish_calibration, after that launch (synchronous, once per geometry and scene
// upload): costs -> order_from_costs -> the order on the device, the slot valid.
int acquire_order(rt_ctx* c, const int32_t (&key)[8], size_t n_tiles, hipStream_t st, rt_ctx::OrderSlot** slot, bool* calibrate);
int finish_calibration(rt_ctx* c, hipStream_t st, rt_ctx::OrderSlot* slot, const OrderParams& p);
// The end of every row launch, behind its last kernel: the timing event, the completion mark where no kernel
// carried it as its stop event (`mark`: the wavefront path), the copy to the caller's buffer when that is host
// memory (the launch rendered into the context's scratch) and the wait for it.
struct HostCopy { void* out; size_t stride; const uint8_t* src; size_t src_stride, row_bytes, n_rows; };   // out null: none
int finish_launch(rt_ctx* c, hipStream_t st, const HostCopy& hc, bool mark);
// What the side entries (k_aa.hip, k_ortho.hip, k_points.hip, k_stats.hip, k_hits.hip, k_paths.hip) refuse first, in
// this order: a null context or argument (args: the entry's other required pointers are there), a context without a
// scene, a two-eye scene (two_eye: the entry's name where it is not built for one, else null) and the depth
// (max_depth, null for an entry that takes none or checks something else first: a negative one becomes the context's,
// and none may pass RT_MAX_DEPTH_CAP, the frames a lane keeps).
inline int side_depth_ok(const rt_ctx* c, int32_t* max_depth) {
  if (*max_depth < 0) *max_depth = c->max_depth;
  if (*max_depth > RT_MAX_DEPTH_CAP) return fail(RT_ERR_UNSUPPORTED, "max_depth %d > %d", *max_depth, RT_MAX_DEPTH_CAP);
  return RT_OK;
}
inline int side_entry_ok(const rt_ctx* c, bool args, const char* two_eye, int32_t* max_depth) {
  if (!c || !args) return fail(RT_ERR_INVALID, "null argument");
  if (!c->uploaded) return fail(RT_ERR_INVALID, "no scene uploaded to this context");
  if (two_eye && c->views.kind)
    return fail(RT_ERR_UNSUPPORTED, "%s is not built for a two-eye scene (stereoscopic / anaglyph camera)", two_eye);
  return max_depth ? side_depth_ok(c, max_depth) : RT_OK;
}
// The launch bracket of the side entries.  begin_launch: the
// timing pair's start event; what an entry keeps out of rt_ctx_last_kernel_ms (memsets of its sums) it enqueues
// first.  end_launch, behind the entry's last kernel: the launch error, the stop event, the completion mark.
inline int begin_launch(rt_ctx* c, hipStream_t st) { if (c->timing) RT_HIP(hipEventRecord(c->ev0, st)); return RT_OK; }
inline int end_launch(rt_ctx* c, hipStream_t st) { RT_HIP(hipGetLastError()); return finish_launch(c, st, HostCopy{}, true); }
// The host-or-device planes of a side entry.  The entry registers them (add_*: the plane's index), then reserve()s:
// every pointer is classified once, a device plane with an `align` is checked (pointer and stride), the host planes
// and the entry's own tables get 256-aligned offsets in the context's scratch, ensure_scratch runs ONCE for the
// total -- it may free and reallocate the buffer, so no pointer into it is formed before -- and the host inputs are
// copied in on st.  Only then ptr() and stride() say what the kernel takes: a device plane as the caller passed it,
// a host plane as packed rows in the scratch.  finish(): the host outputs' copies back on st, and a wait for st
// exactly when a plane was staged or the entry reads something of its own back (must_sync).
struct Stager {
  // p null: a plane not asked for (ptr() null, nothing staged); a contiguous array is one row of row_bytes.
  int add_out(void* p, size_t stride, size_t row_bytes, size_t n_rows, size_t align, const char* what) {
    return add({p, stride, row_bytes, n_rows, align, what, OUT, true, 0});
  }
  int add_in(const void* p, size_t stride, size_t row_bytes, size_t n_rows, size_t align, const char* what) {
    return add({const_cast<void*>(p), stride, row_bytes, n_rows, align, what, IN, true, 0});
  }
  int add_scratch(size_t bytes) { return add({nullptr, bytes, bytes, 1, 0, "", TABLE, false, 0}); }
  int reserve(rt_ctx* c, hipStream_t st);
  template <class T = uint8_t>
  T* ptr(int k) const { return (T*)(pl[k].dev ? pl[k].p : base + pl[k].off); }
  size_t stride(int k) const { return pl[k].dev ? pl[k].stride : pl[k].row_bytes; }
  int finish(hipStream_t st, bool must_sync);

 private:
  enum Kind { OUT, IN, TABLE };
  struct Plane { void* p; size_t stride, row_bytes, n_rows, align; const char* what; Kind kind; bool dev; size_t off; };
  int add(const Plane& q) { pl[n] = q; return n++; }
  Plane pl[6];                                   // the most an entry has: six (rt_ray_paths)
  int n = 0;
  uint8_t* base = nullptr;
  bool staged = false;
};
void drop_order(rt_ctx::OrderSlot& s);         // frees an order table (hipFree waits for its readers)
void drop_orders(rt_ctx* c);
void reset_order_choices(rt_ctx* c);           // a same-structure upload keeps the orders; the ray-tree wavefront choice is timed again
// k_masks.hip: the tile-mask tables
void drop_masks(rt_ctx* c);                    // every table (upload, free): hipFree waits for their readers
bool masks_usable(const rt_ctx* c);            // the uploaded scene has a mask scene (LaunchFacts::masks_ok)
// The mask table's slot of the geometry (a0..a3: y_first, band_rows, band_pitch, n_rows) for a launch on st, filled on st first if it
// is new since the upload
int mask_slot(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, size_t n_tiles, rt_ctx::MaskSlot** out);
// The dispatch records (RecSlot) of a launch of n_entries order entries (d_order of calibration order_id; null and
// 0: the identity) whose mask table is ms's, gathered on st first if the masks or the order are new.
// lean: with the lean bits (RT_OPT_LEAN_TILES), set by the gather and cleared again by the program's check kernel
// where a tile fails it, both on st ahead of the table's event; the context holds that kernel (LaunchPlan::lean).
// traced: the same kernel's trace pass instead (RT_OPT_TRACED_MASKS, LaunchPlan::traced): it narrows every entry's
// words to what its pixels' rays hit and sets the lean bits itself (lean: entries may say lean); the sky and lean
// counts are taken behind it.  traced: 0 no pass, 1 the floor-only entries, 2 the entries with an object pixel too
// (LaunchPlan::traced_objects); a table is keyed by the form.
int launch_records(rt_ctx* c, hipStream_t st, const rt_ctx::MaskSlot* ms, const int32_t* d_order, uint64_t order_id,
                   uint32_t n_entries, bool lean, int traced, const RtTileRec** table, const void** rslot = nullptr);
void drop_records(rt_ctx* c);                  // every record table (upload, free)
// How many of a record table's entries say sky (rslot as launch_records gave it, rec_id its RecSlot::rec_id);
// -1: the table has been dropped since, -2: its gather has not completed yet.  Never waits.
int64_t record_sky_entries(rt_ctx* c, const void* rslot, uint64_t rec_id, uint32_t* n_entries);
int64_t record_lean_entries(rt_ctx* c, const void* rslot, uint64_t rec_id);   // the entries that say lean, likewise
// The run of entries [*first, *end) that holds every lean entry of the table, once its check has completed (true;
// *end == *first: no entry is lean); false until then.  Never waits.
bool record_lean_range(const void* rslot, uint32_t* first, uint32_t* end);
uint64_t record_id(const void* rslot);
size_t put_mask_scene(const FlatScene& f, std::vector<uint8_t>& blob, bool* ok);   // appends the RtTileMaskScene
// A grow-only device buffer of the context: at least `need` bytes at p.  Growing frees the old buffer first (hipFree
// waits for the launches that read it); a failed allocation leaves p null and have 0.
int grow_device(void*& p, size_t& have, size_t need);
int ensure_scratch(rt_ctx* c, size_t bytes);   // the scratch for host-pointer launches, through grow_device
bool is_device_ptr(const void* p);
// Diagnostic switches read from the environment exist only in a diagnostic build (make diag
// DIAG=-DRT_DIAG_ENV): RT_TILE_ORDER_DEBUG (rt_ctx.hip / k_rows.hip: tile-cost statistics and the
// kernel each calibration picked, on stderr) and scene.cpp's flattening switches.  The product
// reads no environment variable.
bool diag_env(const char* name);
// k_wavefront.hip: the wavefront path for the rows of a band layout (wf_plan.h plan_wavefront decides, this carries out)
int launch_wavefront(rt_ctx* c, hipStream_t st, WfRows rows, int max_depth, uint8_t* target, size_t tstride, bool f64,
                     int rgbi, size_t n_tiles, int retry = 0);
// k_stereo.hip: a two-eye scene's row launch (launch_bands' arguments after its checks)
int launch_views(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, int max_depth, uint8_t* target, size_t tstride,
                 bool f64, int rgbi, const HostCopy& hc);
// The facts of a row launch that the context holds (launch_bands and launch_views add the launch's own)
LaunchFacts launch_facts(const rt_ctx* c, int max_depth, bool f64, size_t n_tiles, const rt_ctx::OrderSlot* slot, bool calibrate);
// Completion marks (rt_ctx.hip): record one after every launch of the context on stream st; wait for all
int mark_event(rt_ctx* c, hipStream_t st, hipEvent_t* ev);   // the event a launch on st binds as its stop event
int mark_launch(rt_ctx* c, hipStream_t st);                  // record it after work enqueued on st (other launches)
int wait_launches(rt_ctx* c);
// spec_ctx.hip: the specialised programs of the uploaded scene -- the request to the compile pool
// (asynchronous), the load once compiled (at the next launch, or spec_wait), release
void spec_prepare(rt_ctx* c, bool retry = false);   // describe and request c's programs (spec.level, spec.flat); returns at once
int spec_poll(rt_ctx* c);                           // load them if compiled: RT_OK, or RT_PENDING (spec.error on failure)
int spec_wait(rt_ctx* c, double timeout_ms);        // block (< 0: no limit) then spec_poll
void spec_drop(rt_ctx* c);                          // unload + release (no launch of c may be in flight)
std::string spec_lean_note(const rt_ctx* c);        // why launches take no lean kernel although the program may hold them ("": no reason)
// The loaded row kernel of `kind` for (f64, cal), or null (the generic kernels run).
inline hipFunction_t spec_fn(const rt_ctx* c, int kind, bool f64, bool cal) {
  return c->spec.loaded ? c->spec.slots[kind][f64 ? 1 : 0][cal ? 1 : 0].function : nullptr;
}
// the sample programs (kind: SPEC_POINTS, SPEC_AA)
int spec_samples_wait(rt_ctx* c, double timeout_ms);   // request, block (< 0: no limit), load: RT_OK / RT_PENDING
// The kernel of a points / AA call about to launch (the context's device current): requests the programs on the
// first call, polls, and returns the loaded kernel or null (the generic one runs); sets spec.last_sample.
hipFunction_t spec_sample_kernel(rt_ctx* c, int kind);
std::string spec_sample_info(rt_ctx* c);            // rt_ctx_sample_kernel_info's text
}  // namespace rt
