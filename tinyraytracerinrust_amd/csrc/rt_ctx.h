// rt_ctx.h -- the device context behind the C ABI (include/rt_abi.h: rt_ctx_*), shared by the
// host halves of the kernel translation units: rt_ctx.hip (create / upload / options / streams),
// k_rows.hip (the row kernels' launches), k_stereo.hip (two-eye scenes' launches), k_wavefront.hip,
// k_views.hip.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "rt_blob.h"
#include "scene.h"

namespace rt { struct SpecJob; }        // spec.hip: one program's compile, shared by the contexts that want it

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
  int tile_masks = 1;                   // rt_ctx_set_option(RT_OPT_TILE_MASKS): 0 never, 1 where they pay (OrderSlot::masks_pay), 2 always
  bool masks_ok = false;                // the uploaded scene has a mask scene in its blob (<= 32 objects)
  const void* d_mask_scene = nullptr;   // RtTileMaskScene in the blob
  bool last_masked = false;             // the last row launch passed a mask table (rt_ctx_kernel_info)
  // Scene-specialised row kernels (spec.hip, rt_ctx_set_option(RT_OPT_SPECIALIZE)): hipRTC compiles
  // rt_device.h with this scene's tables as constexpr data, in the background (the library's compile
  // pool); launches take them once they are loaded (spec_poll), the generic kernels until then.
  int spec_on = 1;                      // RT_OPT_SPECIALIZE: 0 off, 1 (default) product launches, 2 every row launch
  std::string spec_src;                 // the program's prelude (spec_source, or a registered family's)
  int spec_mode = 0;                    // RT_MODE_* of the uploaded scene
  bool spec_fc = false;                 // the program's clamp form (RtDevScene::colour_fast)
  bool spec_deferred = false;           // the program also holds the deferred kernels
  bool spec_fits = false;               // small enough to specialise (RT_SPEC_MAX_OBJECTS / _LEAVES)
  hipModule_t spec_mod = nullptr;       // non-null once the kernels are loaded (null: generic kernels)
  hipModule_t spec_mods[16] = {};       // one module per specialised kernel, on this context's device
  hipFunction_t spec_rows[2][2] = {};   // [f64][cal]
  hipFunction_t spec_rows_nm[2][2] = {};   // [f64][cal]: the megakernel compiled WITHOUT the tile-mask operand (a null
                                        // table folded at compile time: the walks of a program without masks), for
                                        // launches that take no table; reflection-only single-scene programs only
  hipFunction_t spec_def[2][2] = {};    // [f64][cal]
  hipFunction_t spec_views[2][2] = {};  // [f64][cal]: the view megakernel (two-eye scenes; their programs hold nothing else)
  bool spec_two_eyes = false;           // the program is a two-eye scene's (spec_flags): view kernels only
  hipFunction_t spec_prim[2][2] = {};   // [f64][cal]: the primary-ray kernel (max_depth 0 launches)
  uint64_t spec_hash = 0;               // FNV-1a of the prelude (kernel info only; caches compare full texts)
  double spec_compile_ms = 0.0;         // the hipRTC time of the loaded programs (0: read from the disk cache)
  int spec_family = 0;                  // > 0: the program of a registered scene family of that many members
  std::shared_ptr<rt::FlatScene> spec_flat;   // the uploaded scene's tables (texels dropped): the program is
                                        // chosen when the option is set (families registered since the upload)
  std::vector<std::shared_ptr<rt::SpecJob>> spec_jobs;   // programs requested, not yet loaded (one per kernel)
  std::string spec_error;               // why the context keeps the generic kernels although spec_on (kernel info)
  std::string spec_note;                // " [process cache]" / " [disk cache]"
  std::string spec_res;                 // the loaded megakernel's resources (kernel info)
  double spec_t0 = 0.0;                 // when the programs were requested (steady clock, ms)
  double spec_ready_ms = 0.0;           // request -> loaded, ms
  // The sample programs (spec.hip rt_spec_points / rt_spec_aa, RT_OPT_SPEC_SAMPLES): the specialised kernels of
  // rt_render_points_f64 ([0]) and of rt_antialias' trace passes ([1]), a job set of their own beside spec_jobs.
  // Requested by the first such call after an upload (and by every later upload once a context has asked),
  // behind the row programs in the pool; each path loads, fails and is reported on its own, and nothing here
  // touches the row programs' state above.
  int samp_on = 1;                      // RT_OPT_SPEC_SAMPLES
  bool samp_wanted = false;             // a points / AA call (or rt_ctx_spec_wait_samples) has asked: uploads request them
  std::shared_ptr<rt::SpecJob> samp_jobs[2];   // requested, not yet loaded
  hipModule_t samp_mods[2] = {};
  hipFunction_t samp_fn[2] = {};        // non-null once loaded (null: the generic kernel)
  std::string samp_error[2];            // why a path stays generic although requested
  std::string samp_res[2];              // a loaded kernel's resources, compile time and provenance (sample kernel info)
  bool samp_cached[2] = {};             // the code object existed in the process when it was requested
  const char* last_sample = "none";     // what the last points / AA trace launch ran (rt_ctx_sample_kernel_info)
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

#define RT_TRY(call)                                                                   \
  do {                                                                                 \
    const int rc_ = (call);                                                            \
    if (rc_) return rc_;                                                               \
  } while (0)

#ifndef RT_SPEC_MAX_OBJECTS
#define RT_SPEC_MAX_OBJECTS 32
#endif
#ifndef RT_SPEC_MAX_LEAVES
#define RT_SPEC_MAX_LEAVES 48
#endif
#define RT_SPEC_MAX_FAMILIES 16

namespace rt {
// rt_ctx.hip
void drop_order(rt_ctx::OrderSlot& s);         // frees an order table (hipFree waits for its readers)
void drop_orders(rt_ctx* c);
void reset_order_choices(rt_ctx* c);           // a same-structure upload keeps the orders; the ray-tree wavefront choice is timed again
// k_masks.hip: the tile-mask tables
void drop_masks(rt_ctx* c);                    // every table (upload, free): hipFree waits for their readers
int tilemask_plane(const FlatScene& f);        // the mask plane's object index, -1: none
// The table of the geometry (a0..a3 as launch_wavefront) for a launch on st, filled on st first if it is new
// since the upload; *table = nullptr when the context takes no masks.
// (*mslot: the table's slot, for launch_records)
int launch_masks(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, size_t n_tiles, const uint32_t** table,
                 const void** mslot = nullptr);
// The dispatch records (RecSlot) of a launch of n_entries order entries (d_order of calibration order_id; null and
// 0: the identity) whose mask table is mask_slot's, gathered on st first if the masks or the order are new.
int launch_records(rt_ctx* c, hipStream_t st, const void* mask_slot, const int32_t* d_order, uint64_t order_id,
                   uint32_t n_entries, const RtTileRec** table);
void drop_records(rt_ctx* c);                  // every record table (upload, free)
size_t put_mask_scene(const FlatScene& f, std::vector<uint8_t>& blob, bool* ok);   // appends the RtTileMaskScene
int ensure_scratch(rt_ctx* c, size_t bytes);   // grow-only device scratch for host-pointer launches
bool is_device_ptr(const void* p);
// Diagnostic switches read from the environment exist only in a diagnostic build (make diag
// DIAG=-DRT_DIAG_ENV): RT_TILE_ORDER_DEBUG (rt_ctx.hip / k_rows.hip: tile-cost statistics and the
// kernel each calibration picked, on stderr) and scene.cpp's flattening switches.  The product
// reads no environment variable.
bool diag_env(const char* name);
// k_wavefront.hip: the wavefront path for rows (y_first, band_rows, band_pitch, n_rows) = a0..a3
int launch_wavefront(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, int max_depth, uint8_t* target,
                     size_t tstride, bool f64, int rgbi, size_t n_tiles, int retry = 0);
// k_stereo.hip: a two-eye scene's row launch (launch_bands' arguments after its checks; out / stride = the
// caller's buffer when it is host memory, target the context's scratch then)
int launch_views(rt_ctx* c, hipStream_t st, int a0, int a1, int a2, int a3, int max_depth, uint8_t* target, size_t tstride,
                 bool f64, int rgbi, void* host_out, size_t host_stride, size_t row_bytes);
// Completion marks (rt_ctx.hip): record one after every launch of the context on stream st; wait for all
int mark_event(rt_ctx* c, hipStream_t st, hipEvent_t* ev);   // the event a launch on st binds as its stop event
int mark_launch(rt_ctx* c, hipStream_t st);                  // record it after work enqueued on st (other launches)
int wait_launches(rt_ctx* c);
// spec.hip: the specialised programs of the uploaded scene -- flags (at upload, cheap), the request to the
// compile pool (asynchronous), the load once compiled (at the next launch, or spec_wait), release
void spec_flags(const FlatScene& f, rt_ctx* c);     // the scene's mode, clamp form, size limits
bool same_structure_flat(const FlatScene& a, const FlatScene& b);   // spec.hip: a scene family's structure test
void spec_prepare(rt_ctx* c, bool retry = false);   // request c's programs (spec_on, spec_flat); returns at once
int spec_poll(rt_ctx* c);                           // load them if compiled: RT_OK, or RT_PENDING (spec_error on failure)
int spec_wait(rt_ctx* c, double timeout_ms);        // block (< 0: no limit) then spec_poll
void spec_drop(rt_ctx* c);                          // unload + release (no launch of c may be in flight)
const char* spec_compiler();                        // which hipRTC compiles the programs
// the sample programs (path 0: points, 1: the anti-aliasing trace)
enum { RT_SAMPLE_POINTS = 0, RT_SAMPLE_AA = 1 };
void spec_samples_request(rt_ctx* c, bool retry = false);   // ask the pool for them (no-op where they do not apply)
void spec_samples_poll(rt_ctx* c);                  // load what has compiled (non-blocking)
int spec_samples_wait(rt_ctx* c, double timeout_ms);   // request, block (< 0: no limit), load: RT_OK / RT_PENDING
// The kernel of a points / AA call about to launch (the context's device current): requests the programs on the
// first call, polls, and returns the loaded kernel or null (the generic one runs); sets last_sample.
hipFunction_t spec_sample_kernel(rt_ctx* c, int path);
std::string spec_sample_info(rt_ctx* c);            // rt_ctx_sample_kernel_info's text
}  // namespace rt
