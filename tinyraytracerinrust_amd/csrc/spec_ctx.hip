// spec_ctx.hip -- a context's scene-specialised kernels (spec.h, rt_ctx.h rt_ctx::Spec): its slots' request,
// load, wait and drop.  The only unit of the four that knows a context or a module.
//
// Life of a program:
//   * rt_ctx_upload REQUESTS the scene's row programs and returns at once (spec_prepare): the pool compiles
//     them (or finds them in the process cache / the on-disk cache) while the context renders with the
//     generic kernels;
//   * the first launch after the compile finished loads the code objects on the context's device and
//     every later launch takes them (k_rows.hip launch_bands -> spec_poll); rt_ctx_spec_wait blocks
//     for them (hosts that want the specialised kernels from their first timed frame, and tests);
//   * a code object the guard refused, or a failed compile, never fails an upload: the context keeps the
//     generic kernels and rt_ctx_kernel_info says why;
//   * the sample programs (rt_render_points_f64 and rt_antialias' trace passes, RT_OPT_SPEC_SAMPLES) are a
//     second job set with the same life, requested by the first such call after an upload and loaded,
//     refused and reported per kernel.
#include <algorithm>
#include <chrono>

#include "rt_ctx.h"

namespace rt {

using SpecSlot = rt_ctx::SpecSlot;

static SpecSlot& slot_of(rt_ctx* c, const SpecKernel& k) { return c->spec.slots[k.kind][k.f64][k.cal]; }

static void slot_request(rt_ctx* c, const SpecKernel& k, bool retry) {
  SpecSlot& s = slot_of(c, k);
  s.error.clear();
  s.job = spec_request(spec_program_text(c->spec.prog, k), spec_bound(c->spec.prog, k.kind), retry, &s.cached);
}

// The finished job's code object onto the context's device: the slot's module, function and resources, or
// its error.  The job is released either way.
static bool slot_load(SpecSlot& s, const SpecKernel& k) {
  const std::shared_ptr<SpecJob> j = std::move(s.job);
  s.error = job_error(*j);
  if (!s.error.empty()) return false;
  hipError_t e = hipModuleLoadData(&s.module, j->code.code.data());
  if (e == hipSuccess) e = hipModuleGetFunction(&s.function, s.module, spec_kernel_name(k).c_str());
  if (e != hipSuccess) {
    if (s.module) (void)hipModuleUnload(s.module);
    s.module = nullptr;
    s.function = nullptr;
    s.error = std::string("loading the specialised code object failed: ") + hipGetErrorString(e);
    return false;
  }
  char b[160];
  snprintf(b, sizeof b, "%d VGPRs (%d spilled), %d B/lane scratch", j->code.vgprs, j->code.vspill, j->code.scratch);
  s.res = b;
  return true;
}

// Unload and release the slots of the row kinds, or of the sample kinds.
static void slots_drop(rt_ctx* c, bool samples) {
  for (int kind = 0; kind < SPEC_KINDS; ++kind) {
    if (spec_is_sample(kind) != samples) continue;
    for (auto& by_cal : c->spec.slots[kind])
      for (SpecSlot& s : by_cal) {
        if (s.module) (void)hipModuleUnload(s.module);
        s = SpecSlot();                                     // drops this context's interest in its job
      }
  }
}

// Blocks for the requested jobs among ks with one deadline (< 0: none); false: not all finished in time.
static bool slots_wait(rt_ctx* c, const std::vector<SpecKernel>& ks, double timeout_ms) {
  std::vector<std::shared_ptr<SpecJob>> jobs;
  for (const SpecKernel& k : ks)
    if (slot_of(c, k).job) jobs.push_back(slot_of(c, k).job);
  return jobs_wait(jobs, timeout_ms);
}

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void rows_drop(rt_ctx* c) {
  slots_drop(c, false);
  c->spec.pending = c->spec.loaded = false;
  c->spec.error.clear();
}

void spec_drop(rt_ctx* c) {
  slots_drop(c, true);                                      // (samples_wanted stays: a context that asked keeps asking)
  rows_drop(c);
}

static void spec_samples_request(rt_ctx* c, bool retry = false);

void spec_prepare(rt_ctx* c, bool retry) {
  rt_ctx::Spec& S = c->spec;
  rows_drop(c);
  S.note.clear();
  if (!S.flat) return;
  S.prog = spec_describe(*S.flat, S.level);
  if (!S.level || !S.prog.fits) return;
  bool all_done = true;
  for (const SpecKernel& k : spec_kernels(S.prog, SPEC_SET_CONTEXT)) {
    slot_request(c, k, retry);
    all_done = all_done && slot_of(c, k).cached;
  }
  S.pending = true;
  if (all_done) S.note = " [process cache]";
  S.t0 = now_ms();
  // a context whose points / AA calls asked for the sample programs before: behind the row programs in the queue
  if (S.samples_wanted) spec_samples_request(c, retry);
}

// The lean kernels (RT_OPT_LEAN_TILES) are requested with the row programs, behind them in the pool, but the row
// programs do not wait for them: each loads when its compile has finished (launches run without lean tiles until
// both are there, launch_plan.h has_lean), and one that fails only leaves its slot empty.
static bool is_lean(const SpecKernel& k) { return spec_kind(k.kind).held == SpecKindRow::LEAN; }
static void lean_poll(rt_ctx* c) {
  for (const SpecKernel& k : spec_kernels(c->spec.prog, SPEC_SET_LEAN)) {
    SpecSlot& s = slot_of(c, k);
    if (s.job && job_finished(s.job.get())) (void)slot_load(s, k);
  }
}

// The row programs load all or nothing: one failure drops them and says why.
int spec_poll(rt_ctx* c) {
  rt_ctx::Spec& S = c->spec;
  if (!S.pending) {
    if (S.loaded) lean_poll(c);
    return RT_OK;
  }
  std::vector<SpecKernel> ks;
  for (const SpecKernel& k : spec_kernels(S.prog, SPEC_SET_CONTEXT))
    if (!is_lean(k)) ks.push_back(k);
  for (const SpecKernel& k : ks)
    if (!job_finished(slot_of(c, k).job.get())) return RT_PENDING;
  for (const SpecKernel& k : ks) {
    const std::string err = job_error(*slot_of(c, k).job);
    if (err.empty()) continue;
    rows_drop(c);
    S.error = err;
    return RT_OK;
  }
  double ms = 0.0;
  bool disk = false;
  for (const SpecKernel& k : ks) {
    SpecSlot& s = slot_of(c, k);
    ms = std::max(ms, s.job->code.compile_ms);
    disk = disk || s.job->code.from_disk;
    if (slot_load(s, k)) continue;
    const std::string err = s.error;
    rows_drop(c);                                           // the sample programs are a job set of their own
    S.error = err;
    return RT_OK;
  }
  S.pending = false;
  S.loaded = true;
  S.hash = fnv1a(S.prog.src);
  S.compile_ms = ms;
  S.res = slot_of(c, ks[0]).res;
  if (disk && S.note.empty()) S.note = " [disk cache]";
  S.ready_ms = now_ms() - S.t0;
  lean_poll(c);
  // Orders built while the generic kernels ran may have chosen the deferred kernel for a tail-bound
  // launch (split entries); with the specialised megakernel loaded that choice no longer pays
  // (k_rows.hip): those geometries calibrate again.
  for (auto& s : c->order)
    if (s.valid && s.deferred) drop_order(s);
  return RT_OK;
}

// (the lean kernels too, also when a launch has loaded the row programs already: a host that waits gets lean
// tiles from its next frame on)
int spec_wait(rt_ctx* c, double timeout_ms) {
  if ((c->spec.pending || c->spec.loaded) && !slots_wait(c, spec_kernels(c->spec.prog, SPEC_SET_CONTEXT), timeout_ms))
    return RT_PENDING;
  return spec_poll(c);
}

// rt_ctx_kernel_info's words on the lean kernels of a loaded program that may hold them: "" where all is well
std::string spec_lean_note(const rt_ctx* c) {
  if (!c->spec.loaded) return "";
  for (const SpecKernel& k : spec_kernels(c->spec.prog, SPEC_SET_LEAN)) {
    const SpecSlot& s = c->spec.slots[k.kind][k.f64][k.cal];
    if (s.function) continue;
    if (s.job) return " (the lean kernels are compiling in the background)";
    if (!s.error.empty()) return " (" + spec_kernel_name(k) + " failed: " + s.error + ")";
  }
  return "";
}

// ---- the sample programs: loaded, failed and reported per kernel -----------------------------------
// Why the sample paths of c take no specialised kernel at all ("" where they may).
static std::string spec_samples_excluded(const rt_ctx* c) {
  char b[160];
  if (!c->spec.samples) return "RT_OPT_SPEC_SAMPLES is off";
  if (!c->spec.level) return "RT_OPT_SPECIALIZE is off";
  if (!c->uploaded || !c->spec.flat) return "no scene uploaded";
  if (!c->spec.prog.fits) {
    snprintf(b, sizeof b, "scene too large to specialise: > %d objects or > %d leaves", RT_SPEC_MAX_OBJECTS, RT_SPEC_MAX_LEAVES);
    return b;
  }
  if (c->spec.prog.two_eyes) return "two-eye scene: the view kernels have no specialised sample form";
  return "";
}

static void spec_samples_request(rt_ctx* c, bool retry) {
  if (!spec_samples_excluded(c).empty()) return;
  c->spec.samples_wanted = true;
  for (const SpecKernel& k : spec_kernels(c->spec.prog, SPEC_SET_SAMPLES)) {
    const SpecSlot& s = slot_of(c, k);
    if (s.function || s.job) continue;                      // loaded, or on its way
    if (!s.error.empty() && !retry) continue;               // failed for this upload: the path stays generic
    slot_request(c, k, retry);
  }
}

static void spec_samples_poll(rt_ctx* c) {
  for (const SpecKernel& k : spec_kernels(c->spec.prog, SPEC_SET_SAMPLES)) {
    SpecSlot& s = slot_of(c, k);
    if (!s.job || !job_finished(s.job.get())) continue;
    const SpecCode& code = s.job->code;
    const double ms = code.compile_ms;
    const bool disk = code.from_disk;
    if (!slot_load(s, k)) continue;
    char b[256];
    snprintf(b, sizeof b, "%s of hipRTC %016llx, %s, compiled in %.0f ms%s", spec_kernel_name(k).c_str(),
             (unsigned long long)fnv1a(c->spec.prog.src), s.res.c_str(), ms, s.cached ? " [process cache]" : disk ? " [disk cache]" : "");
    s.res = b;
  }
}

int spec_samples_wait(rt_ctx* c, double timeout_ms) {
  spec_samples_request(c);
  if (!slots_wait(c, spec_kernels(c->spec.prog, SPEC_SET_SAMPLES), timeout_ms)) return RT_PENDING;
  spec_samples_poll(c);
  return RT_OK;
}

hipFunction_t spec_sample_kernel(rt_ctx* c, int kind) {
  c->spec.last_sample = spec_kind(kind).generic;
  if (!spec_samples_excluded(c).empty()) return nullptr;
  spec_samples_request(c);
  spec_samples_poll(c);
  // the program's clamp form is the scene's; RT_OPT_FAST_CLAMP 0 on a min/max-clamp scene keeps the generic kernel
  if ((c->dev.colour_fast != 0 && c->fast_clamp) != c->spec.prog.fc) return nullptr;
  const hipFunction_t fn = c->spec.slots[kind][0][0].function;
  if (fn) c->spec.last_sample = spec_kind(kind).specialised;
  return fn;
}

std::string spec_sample_info(rt_ctx* c) {
  const std::string excluded = spec_samples_excluded(c);
  std::string s;
  for (int kind = 0; kind < SPEC_KINDS; ++kind) {
    if (!spec_is_sample(kind)) continue;
    const SpecSlot& k = c->spec.slots[kind][0][0];
    s += std::string(s.empty() ? "" : "; ") + spec_kind(kind).generic + ": ";
    if (!excluded.empty()) s += "generic (" + excluded + ")";
    else if (k.function && (c->dev.colour_fast != 0 && c->fast_clamp) != c->spec.prog.fc)
      s += "generic (RT_OPT_FAST_CLAMP is off and the program clamps with min/max)";
    else if (k.function) s += "specialised (" + k.res + ")";
    else if (k.job) s += "generic (the specialised kernel is compiling in the background)";
    else if (!k.error.empty()) s += "generic (specialisation failed: " + k.error + ")";
    else s += "generic (not requested yet: no points or anti-aliasing call since the upload)";
  }
  s += std::string("; last sample launch: ") + c->spec.last_sample;
  return s;
}

}  // namespace rt
