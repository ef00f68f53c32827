// spec.h -- what crosses the seams of the scene-specialised kernels' four units (host code only):
//   spec_compile.cpp  hipRTC (the ROCm installation's own), the code-object metadata, the resource guard
//   spec_pool.cpp     the job table, the compile pool, the process and on-disk caches
//   spec_text.cpp     the program texts: prelude, kernel catalogue, scene families, the rt_scene_* entry points
//   spec_ctx.hip      a context's slots: request, load, wait, drop (the only unit with rt_ctx.h and hipModule*)
#pragma once
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "scene.h"

#ifndef RT_SPEC_MAX_OBJECTS
#define RT_SPEC_MAX_OBJECTS 32
#endif
#ifndef RT_SPEC_MAX_LEAVES
#define RT_SPEC_MAX_LEAVES 48
#endif
#define RT_SPEC_MAX_FAMILIES 16

namespace rt {

// ---- the kernel catalogue (spec_text.cpp spec_kinds) ----------------------------------------------
// The row kinds are one job set of a context, loaded all or nothing; the sample kinds a second, per kernel.
enum SpecKind {
  SPEC_ROWS = 0,      // the megakernel of the scene's mode (masked where the program takes tile masks)
  SPEC_DEFERRED,      // the deferred-shadow kernel (reflection-only scenes: their tail-bound launches' choice)
  SPEC_PRIMARY,       // the primary-ray kernel (launches with max_depth 0)
  SPEC_ROWS_NOMASK,   // the megakernel compiled without the tile-mask operand (launches that pass no table)
  SPEC_VIEWS,         // a two-eye scene's view megakernel (its program holds nothing else)
  SPEC_POINTS,        // rt_render_points_f64's kernel
  SPEC_AA,            // rt_antialias' trace passes
  SPEC_LEAN,          // the lean kernel of the megakernel's launches (RT_OPT_LEAN_TILES; rt_bodies.h lean_body)
  SPEC_LEAN_CHECK,    // its check, run once per record table (k_masks.hip launch_records)
  SPEC_KINDS
};
// The known-good scratch bound a code object is held to (spec_compile.cpp spec_guard).
enum SpecBound { SPEC_BOUND_ROWS = 0, SPEC_BOUND_DEFERRED, SPEC_BOUND_TREE };
struct SpecKindRow {
  const char* name;     // the kernel's name; "%d%d" = f64, cal where the kind has variants
  const char* params;   // its parameters, without the mask operand
  const char* local;    // a declaration of its own ahead of the call ("": none)
  const char* body;     // the body template (rt_device.h) ...
  const char* targs;    // ... its template arguments ($M mode, $F f64, $C cal, $X clamp form, $L frame layout,
                        //     $D chain form of the deferred body) ...
  const char* call;     // ... and its arguments ($S the LDS frames or nullptr, $R the dispatch records where taken)
  bool frames;          // declares the LDS frames (rows_lds_doubles of the mode and layout)
  bool masks;           // takes the mask operand, and RT_REC_PARAMS in a reflection-only program
  bool no_tile_masks;   // its program is prefixed with RT_TILE_MASKS 0
  enum { WAVES_MODE, WAVES_PRIMARY, WAVES_DEFERRED, WAVES_LEAN, WAVES_CHECK } waves;   // where amdgpu_waves_per_eu comes from
  bool variants;        // [f64][cal] instantiations (level 2: all four; level 1: the product's one)
  enum { ONE_EYE, REFLECTION, CONTEXT_REFLECTION, TWO_EYES, SAMPLE, LEAN } held;   // which programs hold it (spec_kernels)
  SpecBound bound;      // SPEC_BOUND_ROWS: by the mode (ray trees: SPEC_BOUND_TREE)
  const char* generic;  // last_sample's words for the generic kernel (sample kinds)
  const char* specialised;
  bool no_cal = false;  // variants: [f64] only, no calibrating form ("%d" = f64)
};
const SpecKindRow& spec_kind(int kind);
inline bool spec_is_sample(int kind) { return spec_kind(kind).held == SpecKindRow::SAMPLE; }

// What decides a scene's programs: made by spec_describe from the flattened scene and the level.
struct SpecProgram {
  std::string src;        // the prelude (spec_source, or a registered family's); "" where !fits or level 0
  int mode = 0;           // RT_MODE_* of the scene
  bool fc = false;        // the clamp form (RtDevScene::colour_fast)
  bool two_eyes = false;  // a two-eye scene's: view kernels only
  bool deferred = false;  // also holds the deferred kernels
  bool fits = false;      // small enough to specialise (RT_SPEC_MAX_OBJECTS / _LEAVES)
  int family = 0;         // > 0: the program of a registered scene family of that many members
  bool lean = false;      // may hold the lean kernels: reflection-only, one eye, tilemask_lean_ok (and no family)
  int level = 1;          // RT_OPT_SPECIALIZE: 0 off, 1 the product launches, 2 every row launch
};
SpecProgram spec_describe(const FlatScene& f, int level);
struct SpecKernel { int kind, f64, cal; };
// The kernels of p's programs, in catalogue order: a scene's row programs as rt_scene_precompile, _spec_report
// and _spec_program name them; a CONTEXT's row programs, which add the mask-free megakernel; the sample programs.
// The lean kernels are a set of their own (rt_scene_lean_report) that a context's row programs include.
enum SpecSet { SPEC_SET_SCENE, SPEC_SET_CONTEXT, SPEC_SET_SAMPLES, SPEC_SET_LEAN };
std::vector<SpecKernel> spec_kernels(const SpecProgram& p, SpecSet set);
std::string spec_kernel_name(const SpecKernel& k);
std::string spec_program_text(const SpecProgram& p, const SpecKernel& k);   // prefix + prelude + the one kernel
SpecBound spec_bound(const SpecProgram& p, int kind);
bool same_structure_flat(const FlatScene& a, const FlatScene& b);   // a scene family's structure test
int tilemask_plane(const FlatScene& f);        // k_masks.hip: the mask plane's object index, -1: none
bool tilemask_sky_ok(const FlatScene& f);      // k_masks.hip: a tile whose prim word is 0 is sky (SKY_OK)
bool tilemask_lean_ok(const FlatScene& f);     // k_masks.hip: a record may say lean (LEAN_OK)
uint64_t fnv1a(const std::string& s);

// ---- the compiler (spec_compile.cpp) ---------------------------------------------------------------
struct SpecCode {
  std::vector<char> code;              // the linked code object
  std::string name;                    // the kernel (code-object metadata .name)
  double compile_ms = 0.0;             // the hipRTC compile that made it (0: read from the disk cache)
  bool from_disk = false;
  int vgprs = -1, sgprs = -1, scratch = -1, vspill = -1, occupancy = -1;   // code-object metadata (occupancy: VGPR-limited)
};
struct SpecCompiler {
  std::string origin;                  // which hipRTC: the kernel info's "compiler" note
  bool rocm = false;                   // the ROCm installation's own (the only one the guard lets compile)
  std::string identity;                // origin + the library file's real path, size and mtime (disk-cache key)
};
const SpecCompiler& spec_compiler();
std::string spec_build_identity();     // the disk-cache identity: compiler, embedded headers, options
int spec_compile(const std::string& src, SpecCode* out, std::string* err);
void code_resources(SpecCode* c);      // name and resource use from the code object's metadata
int spec_guard(const SpecCode& c, SpecBound bound, std::string* err);

// ---- the pool (spec_pool.cpp) ----------------------------------------------------------------------
enum { SPEC_QUEUED = 0, SPEC_RUNNING, SPEC_DONE, SPEC_FAILED, SPEC_CANCELLED };
// One program (prelude + one kernel), keyed by its full text.  `interest` counts the holders (contexts,
// registered families, callers waiting for it): a job nobody holds when a worker reaches it is
// cancelled, so a host that uploads scene after scene (the reference's animate mode builds every
// frame's scene anew, gui.rs:78-89) only ever compiles what it still renders.
struct SpecJob {
  std::string text;
  SpecBound bound = SPEC_BOUND_ROWS;   // what the guard holds the code object to (a function of the text)
  std::atomic<int> state{SPEC_QUEUED};
  std::atomic<int> interest{0};
  SpecCode code;                       // valid once SPEC_DONE
  std::string error;                   // set once SPEC_FAILED
  uint64_t last_use = 0;
  std::mutex mu;
  std::condition_variable cv;
};
// A token for the program `text`: the process's job for it (queued, running or done), or a new job
// for the pool.  retry: a FAILED job is compiled again.  *was_done: the code object already existed.
std::shared_ptr<SpecJob> spec_request(const std::string& text, SpecBound bound, bool retry = false, bool* was_done = nullptr);
bool job_finished(const SpecJob* j);
bool job_wait(SpecJob* j, double timeout_ms);   // (< 0: no limit); true once it has finished
bool jobs_wait(const std::vector<std::shared_ptr<SpecJob>>& jobs, double timeout_ms);   // all of them, one deadline
std::string job_error(const SpecJob& j);        // why a finished job is not SPEC_DONE ("": it is)

}  // namespace rt
