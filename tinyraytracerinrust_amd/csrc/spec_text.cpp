// spec_text.cpp -- the texts of the scene-specialised programs (spec.h; rt_ctx_set_option(RT_OPT_SPECIALIZE),
// default on): the prelude, the kernel catalogue, the scene families and the rt_scene_* entry points.
//
// The generic kernels read the flattened scene (rt_blob.h) from HBM: every hierarchy step, object
// and leaf record is a dependent scalar load, and every branch on a record field (leaf kind,
// transform form, cull kind, filter form) is taken at run time.  A scene is immutable after upload,
// so a program compiles the SAME device code (rt_device.h) once more with the scene's tables as
// constexpr data (RT_SPEC): the hierarchy walk unrolls into nested branches over constant boxes,
// every record field is a literal, and the branches on them fold away.  The arithmetic on ray
// values is unchanged -- the same operations in the same order, -ffp-contract=off, constant folding
// only of values the host computed already -- so the pixels are bit-identical (tests/test_gpu_spec.py).
//
// Each kernel is its own program (prelude + one kernel): the programs compile in parallel (spec_pool.cpp),
// and the inliner sees one kernel per module.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "spec.h"

namespace {

using namespace rt;

// constexpr T NAME[] = { bit_cast<T>(words), ... }: the host record's exact bits (padding included).
// vary (a family program): per 4-byte word, 1 = the word differs between the family's members -- it is
// emitted as 0 and read from the scene's own table (rt_device.h RT_REC), and VARY_NAME lists the mask.
template <class T>
void emit_table(std::string& s, const char* type, const char* name, const std::vector<T>& v,
                const std::vector<uint8_t>* vary = nullptr) {
  static_assert(sizeof(T) % 8 == 0, "spec tables are emitted as 64-bit words");
  constexpr size_t W = sizeof(T) / 8;
  char buf[64];
  s += "constexpr ";
  s += type;
  s += " ";
  s += name;
  s += "[] = {\n";
  std::vector<T> rows(v);
  if (rows.empty()) {                  // no zero-length arrays: one zero record, never read (N_* = 0)
    rows.resize(1);
    memset((void*)rows.data(), 0, sizeof(T));
  }
  for (size_t ri = 0; ri < rows.size(); ++ri) {
    uint64_t w[W];
    memcpy(w, &rows[ri], sizeof(T));
    if (vary && !v.empty())
      for (size_t i = 0; i < 2 * W; ++i)
        if ((*vary)[ri * 2 * W + i]) w[i / 2] &= i % 2 ? 0xffffffffull : 0xffffffff00000000ull;
    s += "  __builtin_bit_cast(";
    s += type;
    s += ", SpecRaw<";
    snprintf(buf, sizeof buf, "%zu", W);
    s += buf;
    s += ">{{";
    for (size_t i = 0; i < W; ++i) {
      snprintf(buf, sizeof buf, "%s0x%llxull", i ? "," : "", (unsigned long long)w[i]);
      s += buf;
    }
    s += "}}),\n";
  }
  s += "};\n";
  if (vary) {
    s += "constexpr uint8_t VARY_";
    s += name;
    s += "[] = {";
    if (v.empty()) s += "0";
    for (size_t i = 0; i < vary->size(); ++i) s += (*vary)[i] ? (i ? ",1" : "1") : (i ? ",0" : "0");
    s += "};\n";
  }
}

// ---- scene families (rt_spec_family_register): one program for scenes of the same structure
// The frames of an animation differ in some numbers (an object's centre and transform, a colour)
// and share everything else -- table sizes, the hierarchy, kinds and flags, most parameters.  A
// family program holds the words every member shares as constants and reads the others from the
// rendering scene's own tables (rt_device.h RT_REC), so one hipRTC compile serves every member.
template <class T>
void vary_words(const std::vector<T>& a, const std::vector<T>& b, std::vector<uint8_t>* m) {
  const size_t n = a.size() * sizeof(T) / 4;
  m->resize(n, 0);
  const uint32_t* x = (const uint32_t*)(const void*)a.data();
  const uint32_t* y = (const uint32_t*)(const void*)b.data();
  for (size_t i = 0; i < n; ++i) (*m)[i] |= x[i] != y[i];
}
template <class T>
bool same_except(const std::vector<T>& a, const std::vector<T>& b, const std::vector<uint8_t>& m) {
  if (a.size() != b.size()) return false;
  const uint32_t* x = (const uint32_t*)(const void*)a.data();
  const uint32_t* y = (const uint32_t*)(const void*)b.data();
  for (size_t i = 0; i < a.size() * sizeof(T) / 4; ++i)
    if (!m[i] && x[i] != y[i]) return false;
  return true;
}
template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct SpecFamily {
  int members = 0;
  FlatScene base;                      // member 0, without its texels
  std::vector<uint8_t> v_obj, v_trav, v_strav, v_leaf, v_light;
  std::string src;                     // the program's prelude
  std::vector<std::shared_ptr<SpecJob>> jobs;   // its compiled kernels, kept resident while registered
};
std::mutex g_family_mu;                // the registered families
std::vector<std::shared_ptr<SpecFamily>> g_families;   // under g_family_mu; newest last
std::vector<std::shared_ptr<SpecFamily>> g_singles;    // "families" of one registered scene: hold its own program

// Same structure: equal table sizes, flags, hierarchy nodes, CSG nodes, filter programs and
// texture records (the family program holds those as plain constants).
bool same_structure(const FlatScene& a, const FlatScene& b) {
  return a.objects.size() == b.objects.size() && a.trav.size() == b.trav.size() && a.strav.size() == b.strav.size() &&
         a.leaves.size() == b.leaves.size() && a.lights.size() == b.lights.size() && same_bytes(a.nodes, b.nodes) &&
         same_bytes(a.prog, b.prog) && same_bytes(a.textures, b.textures) && a.any_transparent == b.any_transparent &&
         a.shadow_early_out == b.shadow_early_out && a.colour_fast == b.colour_fast && a.ray_chains == b.ray_chains;
}
bool family_member(const SpecFamily& F, const FlatScene& f) {
  return same_structure(F.base, f) && same_except(F.base.objects, f.objects, F.v_obj) &&
         same_except(F.base.trav, f.trav, F.v_trav) && same_except(F.base.strav, f.strav, F.v_strav) &&
         same_except(F.base.leaves, f.leaves, F.v_leaf) && same_except(F.base.lights, f.lights, F.v_light);
}

// A diagnostic build's -D switches (Makefile: $(DIAG) as the string RT_SPEC_DIAG_DEFINES) as #define
// lines for the programs' prelude, so the specialised kernels of a diagnostic build are built the way
// its precompiled kernels are (empty in the product build).
#ifndef RT_SPEC_DIAG_DEFINES
#define RT_SPEC_DIAG_DEFINES ""
#endif
std::string diag_prelude() {
  std::string out, w;
  const std::string s = RT_SPEC_DIAG_DEFINES;
  for (size_t i = 0; i <= s.size(); ++i) {
    if (i < s.size() && s[i] != ' ') { w += s[i]; continue; }
    if (w.rfind("-D", 0) == 0 && w.size() > 2) {
      const size_t eq = w.find('=');
      out += "#define " + (eq == std::string::npos ? w.substr(2) : w.substr(2, eq - 2) + " " + w.substr(eq + 1)) + "\n";
    }
    w.clear();
  }
  return out;
}

// The program's prelude: the scene's tables as constexpr data, then the device code.  fam: the
// family's program (the words that differ between members zeroed, their masks emitted).
// (The first line is part of every program's text, and so of the on-disk cache's file names: it stays.)
std::string spec_source(const FlatScene& f, const SpecFamily* fam) {
  std::string s;
  char buf[256];
  s += std::string("// scene-specialised row kernels (spec.hip)\n#define RT_SPEC 1\n") + diag_prelude() +
       (fam ? "#define RT_SPEC_FAMILY 1\n" : "") + "#define RT_TILE_W " + std::to_string(RT_TILE_W) +
       "\n#include \"rt_blob.h\"\n";
  s += "template <int N> struct SpecRaw { unsigned long long w[N]; };\nnamespace rt_spec {\n";
  snprintf(buf, sizeof buf,
           "constexpr int N_OBJECTS = %d, N_LIGHTS = %d, N_TRAV = %d, N_STRAV = %d, SHADOW_EARLY_OUT = %d;\n",
           (int)f.objects.size(), (int)f.lights.size(), (int)f.trav.size(), (int)f.strav.size(), f.shadow_early_out);
  s += buf;
  // the tile masks' plane (rt_tilemask.h): the object the mask tables' shadow and refl words were built for
  // (a family program takes no masks: its members' planes and boxes differ)
  snprintf(buf, sizeof buf, "constexpr int MASK_PLANE = %d;\n", fam ? -1 : tilemask_plane(f));
  s += buf;
  // sky tiles (rt_device.h rows_entry): every object is boxed or the mask plane, so prim words can be 0
  s += std::string("constexpr bool SKY_OK = ") + (!fam && tilemask_sky_ok(f) ? "true" : "false") + ";\n";
  // lean tiles (rt_bodies.h rows_entry, lean_body): a record may carry the lean bit, the megakernel returns on it
  s += std::string("constexpr bool LEAN_OK = ") + (!fam && tilemask_lean_ok(f) ? "true" : "false") + ";\n";
  emit_table(s, "RtObject", "OBJECTS", f.objects, fam ? &fam->v_obj : nullptr);
  emit_table(s, "RtTrav", "TRAV", f.trav, fam ? &fam->v_trav : nullptr);
  emit_table(s, "RtTrav", "STRAV", f.strav, fam ? &fam->v_strav : nullptr);
  emit_table(s, "RtNode", "NODES", f.nodes);
  emit_table(s, "RtLeaf", "LEAVES", f.leaves, fam ? &fam->v_leaf : nullptr);
  emit_table(s, "RtProg", "PROG", f.prog);
  emit_table(s, "RtLight", "LIGHTS", f.lights, fam ? &fam->v_light : nullptr);
  emit_table(s, "RtTexture", "TEXTURES", f.textures);
  s += "}  // namespace rt_spec\n#include \"rt_device.h\"\n";
  return s;
}

// The frame storage the programs' kernels are instantiated with (rows_lds_doubles<MODE, kl, kp>).
std::string spec_frame_layout() {
  // stack frames in LDS: 4 waves/SIMD leave 10 KB per one-wave workgroup (the generic kernel's 2
  // frames at 5 waves: 4 KB); RT_SPEC_LDS_FRAMES (diagnostic builds) overrides the mode's default
#ifdef RT_SPEC_LDS_FRAMES
  int kl = RT_SPEC_LDS_FRAMES;
#else
  int kl = -1;
#endif
  int kp = -1;                                                  // the wave pool's slots (-1: the mode's default)
#ifdef RT_DIAG_ENV
  if (const char* e = getenv("RT_SPEC_KL")) kl = atoi(e);      // diagnostic builds: A/B of the LDS frames
  if (const char* e = getenv("RT_SPEC_KP")) kp = atoi(e);
#endif
  return std::to_string(kl) + ", " + std::to_string(kp);
}

// The specialised megakernel runs 4 waves/SIMD (128 VGPRs): its unrolled walks keep more values
// live than the generic loop, and at the generic reflection kernel's 5 waves (96 VGPRs) it spilled
// 62 VGPRs; 4 waves measured 4.9 % faster on 4K globes (0.3499 vs 0.3679 ms,
// profiles/r05e_spec_waves_ab.txt).  Diagnostic builds may set RT_SPEC_WAVES.
#ifndef RT_SPEC_WAVES
#define RT_SPEC_WAVES 4
#endif
// Chain-mode programs (the anim120 families: 82 VGPRs, 6 waves/SIMD set by the VGPRs and the 6 KB of
// LDS frames) at 7 waves (72 VGPRs, 11 spilled, a 100-110-slot pool) measured 0.5-1 % slower
// (profiles/r08j_chain_waves_ab.txt).  Diagnostic builds may set RT_SPEC_WAVES_CHAIN.
#ifndef RT_SPEC_WAVES_CHAIN
#define RT_SPEC_WAVES_CHAIN RT_SPEC_WAVES
#endif
// The primary-ray kernel: no frame stack, so its VGPRs (not a fixed budget) set its occupancy.
#ifndef RT_SPEC_WAVES_PRIM
#define RT_SPEC_WAVES_PRIM 4
#endif

// The lean kernels (rt_bodies.h lean_body): one plane hit, its lights and a fold -- 8 waves' registers.
#ifndef RT_SPEC_WAVES_LEAN
#define RT_SPEC_WAVES_LEAN 8
#endif
// Their check kernel also holds the trace pass (rt_bodies.h trace_masks_body: two nearest-hit walks, a shadow walk
// and the shading inputs live across them): at the lean kernel's 8 waves (64 VGPRs) it spilled 99 VGPRs, so it
// takes the megakernel's 4.  It runs once per record table.
#ifndef RT_SPEC_WAVES_CHECK
#define RT_SPEC_WAVES_CHECK 4
#endif

// The catalogue: one row per SpecKind (spec.h SpecKindRow), the generic kernels' exact bodies.  The row kernels
// share the generic kernels' parameters; the megakernel and the primary-ray kernel also take the launch
// geometry's tile-mask table (null: all ones) -- and, in a masked program of a reflection-only scene
// (rt_device.h RT_REC_PARAMS: empty elsewhere), its dispatch records; the mask-free megakernel (RT_TILE_MASKS 0:
// the device code without the mask operand, not merely a null table) keeps the signature without them.  The
// sample kernels are one-wave workgroups with the megakernel's occupancy and frame storage and mask-free walks
// (a sample belongs to no tile).
#define ROW_PARAMS                                                                                                    \
  "int y_first, int band_rows, int band_pitch, int n_rows, int max_depth, uint8_t* __restrict__ out, size_t stride, " \
  "const int32_t* __restrict__ order, uint32_t* __restrict__ cost, int rgb"
#define ROW_CALL(depth) "y_first, band_rows, band_pitch, n_rows, " depth ", out, stride, order, cost, rgb, "
using K = SpecKindRow;
const SpecKindRow spec_kinds[SPEC_KINDS] = {
    /* SPEC_ROWS */ {"rt_spec_rows_%d%d", "RtDevScene S, " ROW_PARAMS, "", "rows_body", "$M, $F, $C, $X, $L",
                     "S, " ROW_CALL("max_depth") "$S, masks$R", true, true, false, K::WAVES_MODE, true, K::ONE_EYE,
                     SPEC_BOUND_ROWS, nullptr, nullptr},
    /* SPEC_DEFERRED */ {"rt_spec_def_%d%d", "RtDevScene S, " ROW_PARAMS, "  __shared__ ShadowWin win;\n", "deferred_body",
                         "$F, $C, $X, $D", "S, " ROW_CALL("max_depth") "&win", false, false, false, K::WAVES_DEFERRED, true,
                         K::REFLECTION, SPEC_BOUND_DEFERRED, nullptr, nullptr},
    /* SPEC_PRIMARY */ {"rt_spec_prim_%d%d", "RtDevScene S, " ROW_PARAMS, "", "rows_body", "$M, $F, $C, $X, 0, 0, true",
                        "S, " ROW_CALL("0") "$S, masks$R", false, true, false, K::WAVES_PRIMARY, true, K::ONE_EYE,
                        SPEC_BOUND_ROWS, nullptr, nullptr},
    /* SPEC_ROWS_NOMASK */ {"rt_spec_rows_%d%d", "RtDevScene S, " ROW_PARAMS, "", "rows_body", "$M, $F, $C, $X, $L",
                            "S, " ROW_CALL("max_depth") "$S, nullptr$R", true, true, true, K::WAVES_MODE, true,
                            K::CONTEXT_REFLECTION, SPEC_BOUND_ROWS, nullptr, nullptr},
    /* SPEC_VIEWS */ {"rt_spec_views_%d%d", "RtDevScene S, RtViews VW, " ROW_PARAMS, "", "rows_views_body",
                      "$M, $F, $C, $X, $L", "S, VW, " ROW_CALL("max_depth") "$S", true, false, true, K::WAVES_MODE, true,
                      K::TWO_EYES, SPEC_BOUND_ROWS, nullptr, nullptr},
    /* SPEC_POINTS */ {"rt_spec_points",
                       "RtDevScene S, const double* __restrict__ xy, size_t n, int max_depth, double* __restrict__ out", "",
                       "points_body", "$M, $X, $L", "S, xy, n, max_depth, out, $S", true, false, true, K::WAVES_MODE, false,
                       K::SAMPLE, SPEC_BOUND_ROWS, "points", "points (specialised)"},
    /* SPEC_AA */ {"rt_spec_aa",
                   "RtDevScene S, const uint32_t* __restrict__ edges, const uint32_t* __restrict__ req, uint32_t n, int size, "
                   "double* __restrict__ col, int max_depth",
                   "", "aa_trace_body", "$M, $X, $L", "S, edges, req, n, size, col, max_depth, $S", true, false, true,
                   K::WAVES_MODE, false, K::SAMPLE, SPEC_BOUND_ROWS, "aa trace", "aa trace (specialised)"},
    // the lean kernel takes the megakernel's operands (one argument list serves both launches), the check the
    // launch geometry, the record table it edits and its mode (the check, or the trace pass of RT_OPT_TRACED_MASKS)
    /* SPEC_LEAN */ {"rt_spec_lean_%d", "RtDevScene S, " ROW_PARAMS, "", "lean_body", "$F, $X",
                     "S, y_first, band_rows, band_pitch, n_rows, max_depth, out, stride, rgb$R", false, true, false,
                     K::WAVES_LEAN, true, K::LEAN, SPEC_BOUND_ROWS, nullptr, nullptr, true},
    /* SPEC_LEAN_CHECK */ {"rt_spec_lean_check",
                           "RtDevScene S, int y_first, int band_rows, int band_pitch, int n_rows, RtTileRec* __restrict__ recs, "
                           "int mode, uint32_t keep_bit",
                           "", "lean_check_body", "$X", "S, y_first, band_rows, band_pitch, n_rows, recs, mode, keep_bit", false, false,
                           false, K::WAVES_CHECK, false, K::LEAN, SPEC_BOUND_ROWS, nullptr, nullptr},
};

// s with every $-placeholder of the catalogue replaced (vars: pairs of letter and text).
std::string expand(const char* s, const std::vector<std::pair<char, std::string>>& vars) {
  std::string out;
  for (; *s; ++s) {
    if (*s != '$') { out += *s; continue; }
    ++s;
    for (const auto& v : vars)
      if (v.first == *s) out += v.second;
  }
  return out;
}

// One kernel of the program, from its catalogue row.
std::string spec_kernel(const SpecProgram& p, const SpecKernel& k) {
  const SpecKindRow& row = spec_kinds[k.kind];
  const bool recs = row.masks && p.mode == RT_MODE_REFL;
  const std::string layout = spec_frame_layout();
  auto tf = [](bool b) { return std::string(b ? "true" : "false"); };
  const std::vector<std::pair<char, std::string>> vars = {
      {'M', std::to_string(p.mode)}, {'F', tf(k.f64)}, {'C', tf(k.cal)}, {'X', tf(p.fc)}, {'L', layout},
      {'D', tf(p.mode != RT_MODE_REFL)}, {'S', row.frames ? "(lds_f64*)s_frames" : "nullptr"}, {'R', recs ? " RT_REC_ARGS" : ""}};
  const std::string waves = row.waves == K::WAVES_DEFERRED  ? "RT_WAVES_PER_EU_DEFERRED"
                            : row.waves == K::WAVES_PRIMARY ? std::to_string(RT_SPEC_WAVES_PRIM)
                            : row.waves == K::WAVES_LEAN    ? std::to_string(RT_SPEC_WAVES_LEAN)
                            : row.waves == K::WAVES_CHECK   ? std::to_string(RT_SPEC_WAVES_CHECK)
                                                            : std::to_string(p.mode == RT_MODE_CHAIN ? RT_SPEC_WAVES_CHAIN : RT_SPEC_WAVES);
  std::string s = "extern \"C\" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(" + waves + "))) void " +
                  spec_kernel_name(k) + "(" + row.params;
  if (row.masks) s += std::string(", const uint32_t* __restrict__ masks") + (recs ? " RT_REC_PARAMS" : "");
  s += std::string(") {\n") + row.local;
  if (row.frames) s += expand("  __shared__ double s_frames[rows_lds_doubles<$M, $L>()];\n", vars);
  return s + "  " + row.body + "<" + expand(row.targs, vars) + ">(" + expand(row.call, vars) + ");\n}\n";
}

// The flags of a flattened scene that decide its program (cheap; no text is generated).
SpecProgram spec_flags(const FlatScene& f, int level) {
  SpecProgram p;
  p.level = level;
  // The walks unroll over every hierarchy node and leaf, twice (nearest hit, shadows), and the
  // shading over every object: code size and compile time grow with the scene (globes.scene, 6
  // objects and 11 leaves: ~15 k instructions, ~3-12 s of hipRTC per kernel).  Larger scenes keep the
  // generic kernels (fractal.scene: 171 objects).
  p.fits = f.objects.size() <= RT_SPEC_MAX_OBJECTS && f.leaves.size() <= RT_SPEC_MAX_LEAVES;
  p.mode = !f.any_transparent ? RT_MODE_REFL : f.ray_chains ? RT_MODE_CHAIN : RT_MODE_TREE;
  p.fc = f.colour_fast != 0;
  p.two_eyes = f.cam_kind != RT_CAMERA_PERSPECTIVE;
  p.deferred = p.mode == RT_MODE_REFL && !p.two_eyes;
  p.lean = p.mode == RT_MODE_REFL && !p.two_eyes && tilemask_lean_ok(f);
  return p;
}

// The prelude of a flattened scene: a registered family's, or its own.
void spec_prelude(const FlatScene& f, SpecProgram* p) {
  {
    std::lock_guard<std::mutex> lk(g_family_mu);
    for (auto it = g_families.rbegin(); it != g_families.rend(); ++it)
      if (family_member(**it, f)) {
        p->src = (*it)->src;
        p->family = (*it)->members;
        return;
      }
  }
  p->src = spec_source(f, nullptr);
}

int copy_out(const std::string& text, char* buf, size_t cap, size_t* len) {
  *len = text.size();
  if (cap > 0) {
    const size_t n = text.size() < cap - 1 ? text.size() : cap - 1;
    memcpy(buf, text.data(), n);
    buf[n] = 0;
  }
  return RT_OK;
}

int not_specialised(const FlatScene& f, bool family) {
  return fail(RT_ERR_UNSUPPORTED, "%s of %zu objects / %zu leaves %s not specialised (limits %d / %d)", family ? "scenes" : "scene",
              f.objects.size(), f.leaves.size(), family ? "are" : "is", RT_SPEC_MAX_OBJECTS, RT_SPEC_MAX_LEAVES);
}

// Programs requested from the pool, and whether each code object existed already.
struct Requested {
  std::vector<std::shared_ptr<SpecJob>> jobs;
  std::vector<bool> was_done;
  void add(const SpecProgram& p, SpecSet set) {
    for (const SpecKernel& k : spec_kernels(p, set)) {
      bool done = false;
      jobs.push_back(spec_request(spec_program_text(p, k), spec_bound(p, k.kind), false, &done));
      was_done.push_back(done);
    }
  }
  // Waits for every job (no limit); the longest fresh compile in *ms (0: all came from a cache); the
  // first failure's status and message.
  int wait(double* ms) const {
    *ms = 0.0;
    for (size_t i = 0; i < jobs.size(); ++i) {
      job_wait(jobs[i].get(), -1.0);
      if (jobs[i]->state.load() != SPEC_DONE) return fail(RT_ERR_UNSUPPORTED, "%s", job_error(*jobs[i]).c_str());
      if (!was_done[i]) *ms = std::max(*ms, jobs[i]->code.compile_ms);
    }
    return RT_OK;
  }
  // One kernel's line each (rt_scene_spec_report / rt_scene_sample_report).
  std::string report() const {
    std::string text;
    for (const auto& j : jobs) {
      const SpecCode& c = j->code;
      char line[512];
      snprintf(line, sizeof line, "%s: vgprs %d spilled %d sgprs %d scratch %d occupancy %d code %zu compile_ms %.0f source %s\n",
               c.name.c_str(), c.vgprs, c.vspill, c.sgprs, c.scratch, c.occupancy, c.code.size(), c.compile_ms,
               c.from_disk ? "disk" : "hiprtc");
      text += line;
    }
    return text;
  }
};

// The level-1 programs of scene s (or its two sample programs), requested and waited for.
int scene_programs(const rt_scene* s, SpecSet set, Requested* r, double* ms) {
  FlatScene f;
  RT_TRY(flatten(*s, &f));
  const SpecProgram p = spec_describe(f, 1);
  if (!p.fits) return not_specialised(f, false);
  if (set == SPEC_SET_SAMPLES && p.two_eyes) return fail(RT_ERR_UNSUPPORTED, "a two-eye scene has no specialised sample kernels");
  r->add(p, set);
  return r->wait(ms);
}

}  // namespace

namespace rt {

const SpecKindRow& spec_kind(int kind) { return spec_kinds[kind]; }

bool same_structure_flat(const FlatScene& a, const FlatScene& b) { return same_structure(a, b); }

SpecProgram spec_describe(const FlatScene& f, int level) {
  SpecProgram p = spec_flags(f, level);
  if (level > 0 && p.fits) spec_prelude(f, &p);
  return p;
}

// RT_OPT_SPECIALIZE 1: the RGBA8 / RGB8 product launches (f64 = 0, cal = 0); 2: the f64 and calibration
// instantiations too (tests: every launch of a parity test then runs specialised).
// A two-eye scene's program holds the view megakernel only (mask-free walks): every launch of such a scene takes
// it, and a perspective scene's program holds none.  The camera reaches the kernels as an argument, so the
// prelude -- and the program -- does not depend on the eyes.
// The masked walks cost a few percent whether a mask rules anything out or not (DESIGN.md "Tile masks"),
// so a context whose megakernel reads masks also holds the megakernel without them -- the same kernel name
// in a module of its own -- and launch_bands takes it for the launches that pass no table; it is requested (in
// the background, like the others) by the context that uploads the scene.
std::vector<SpecKernel> spec_kernels(const SpecProgram& p, SpecSet set) {
  std::vector<SpecKernel> v;
  for (int kind = 0; kind < SPEC_KINDS; ++kind) {
    const SpecKindRow& row = spec_kinds[kind];
    bool held = false;
    switch (row.held) {
      case K::ONE_EYE: held = set != SPEC_SET_SAMPLES && !p.two_eyes; break;
      case K::REFLECTION: held = set != SPEC_SET_SAMPLES && p.deferred; break;
      case K::CONTEXT_REFLECTION: held = set == SPEC_SET_CONTEXT && !p.two_eyes && p.mode == RT_MODE_REFL && !p.family; break;
      case K::TWO_EYES: held = set != SPEC_SET_SAMPLES && p.two_eyes; break;
      case K::SAMPLE: held = set == SPEC_SET_SAMPLES && !p.two_eyes; break;
      case K::LEAN: held = (set == SPEC_SET_CONTEXT || set == SPEC_SET_LEAN) && p.lean && !p.family; break;
    }
    if (set == SPEC_SET_LEAN && row.held != K::LEAN) continue;
    if (!held) continue;
    const int n = row.variants && p.level >= 2 ? 2 : 1;
    for (int f64 = 0; f64 < n; ++f64)
      for (int cal = 0; cal < (row.no_cal ? 1 : n); ++cal) v.push_back({kind, f64, cal});
  }
  return v;
}

std::string spec_kernel_name(const SpecKernel& k) {
  char name[32];
  snprintf(name, sizeof name, spec_kinds[k.kind].name, k.f64, k.cal);   // (a name without %d%d ignores them)
  return name;
}

std::string spec_program_text(const SpecProgram& p, const SpecKernel& k) {
  return (spec_kinds[k.kind].no_tile_masks ? "#define RT_TILE_MASKS 0\n" : "") + p.src + spec_kernel(p, k);
}

SpecBound spec_bound(const SpecProgram& p, int kind) {
  const SpecBound b = spec_kinds[kind].bound;
  return b == SPEC_BOUND_ROWS && p.mode == RT_MODE_TREE ? SPEC_BOUND_TREE : b;
}

}  // namespace rt

// rt_scene_precompile (include/rt_abi.h): the specialised programs of a scene into the process cache,
// no device needed -- a host may compile on a worker thread while it renders with the generic kernels
extern "C" int rt_scene_precompile(const rt_scene* s, double* compile_ms) {
  if (!s) return fail(RT_ERR_INVALID, "null scene");
  Requested r;
  double ms = 0.0;
  // the row programs and the lean kernels a context's row programs include, all requested before any is waited for
  FlatScene f;
  RT_TRY(flatten(*s, &f));
  const SpecProgram p = spec_describe(f, 1);
  int rc = RT_OK;
  if (!p.fits) {
    rc = not_specialised(f, false);
  } else {
    r.add(p, SPEC_SET_SCENE);
    r.add(p, SPEC_SET_LEAN);
    rc = r.wait(&ms);
  }
  if (compile_ms) *compile_ms = ms;
  return rc;
}

// rt_scene_spec_report (include/rt_abi.h): compile (or find) the scene's level-1 programs and describe
// them: the compiler, and per kernel its resource use and how it was obtained
extern "C" int rt_scene_spec_report(const rt_scene* s, char* buf, size_t cap, size_t* len) {
  if (!len || (cap > 0 && !buf)) return fail(RT_ERR_INVALID, "null argument");
  if (!s) return fail(RT_ERR_INVALID, "null scene");
  Requested r;
  double ms = 0.0;
  RT_TRY(scene_programs(s, SPEC_SET_SCENE, &r, &ms));
  // source: how the code object was made -- by hipRTC in this process, or read from the disk cache
  const SpecCompiler& R = spec_compiler();
  return copy_out("compiler: " + R.identity + (R.rocm ? " (the ROCm installation's hipRTC)" : "") + "\n" + r.report(), buf, cap, len);
}

// rt_scene_sample_report (include/rt_abi.h): compile (or find) the scene's two sample programs, no device
// needed, and describe them, one line per kernel in rt_scene_spec_report's format
extern "C" int rt_scene_sample_report(const rt_scene* s, char* buf, size_t cap, size_t* len) {
  if (!s || !len || (cap > 0 && !buf)) return fail(RT_ERR_INVALID, "null argument");
  Requested r;
  double ms = 0.0;
  RT_TRY(scene_programs(s, SPEC_SET_SAMPLES, &r, &ms));
  return copy_out(r.report(), buf, cap, len);
}

// rt_scene_lean_report (include/rt_abi.h): compile (or find) the scene's lean kernels (RT_OPT_LEAN_TILES), no device
// needed, and describe them in rt_scene_spec_report's format; a scene whose programs hold none: no lines
extern "C" int rt_scene_lean_report(const rt_scene* s, char* buf, size_t cap, size_t* len) {
  if (!s || !len || (cap > 0 && !buf)) return fail(RT_ERR_INVALID, "null argument");
  Requested r;
  double ms = 0.0;
  RT_TRY(scene_programs(s, SPEC_SET_LEAN, &r, &ms));
  return copy_out(r.report(), buf, cap, len);
}

// rt_scene_spec_program (include/rt_abi.h): the prelude and every kernel rt_scene_precompile compiles
// (at level 2: with the f64 and calibration instantiations; a scene too large to specialise has a text too)
extern "C" int rt_scene_spec_program(const rt_scene* s, char* buf, size_t cap, size_t* len) {
  if (!s || !len || (cap > 0 && !buf)) return fail(RT_ERR_INVALID, "null argument");
  FlatScene f;
  RT_TRY(flatten(*s, &f));
  SpecProgram p = spec_describe(f, 2);
  if (!p.fits) spec_prelude(f, &p);
  std::string text = p.src;
  for (const SpecKernel& k : spec_kernels(p, SPEC_SET_SCENE)) text += spec_kernel(p, k);
  for (const SpecKernel& k : spec_kernels(p, SPEC_SET_LEAN)) text += spec_kernel(p, k);   // (a context's, where held)
  return copy_out(text, buf, cap, len);
}

// rt_spec_family_register (include/rt_abi.h): specialised programs for n scenes (the frames of an
// animation), one per class of scenes of the same structure and object hierarchy (the frames of
// spinning_globes.scene fall in two: the hierarchy's grouping follows the globes' positions);
// contexts whose scene belongs to a class load its program (spec_describe).
static bool same_hierarchy(const std::vector<RtTrav>& a, const std::vector<RtTrav>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].obj != b[i].obj || a[i].skip != b[i].skip) return false;
  return true;
}
extern "C" int rt_spec_family_register(const rt_scene* const* scenes, int32_t n, double* compile_ms) {
  if (compile_ms) *compile_ms = 0.0;
  if (!scenes || n < 1) return fail(RT_ERR_INVALID, "no scenes");
  std::vector<std::shared_ptr<SpecFamily>> fams;
  FlatScene f;
  for (int32_t i = 0; i < n; ++i) {
    if (!scenes[i]) return fail(RT_ERR_INVALID, "null scene %d", i);
    RT_TRY(flatten(*scenes[i], &f));
    f.texels.clear();
    SpecFamily* F = nullptr;
    for (auto& x : fams)
      if (same_structure(x->base, f) && same_hierarchy(x->base.trav, f.trav) && same_hierarchy(x->base.strav, f.strav)) {
        F = x.get();
        break;
      }
    if (!F) {
      if (fams.size() >= RT_SPEC_MAX_FAMILIES)             // every family is a compile: bounded per call
        return fail(RT_ERR_UNSUPPORTED, "the scenes form more than %d families (structure or object hierarchy differ)",
                    RT_SPEC_MAX_FAMILIES);
      fams.push_back(std::make_shared<SpecFamily>());
      F = fams.back().get();
      F->base = f;
    }
    F->members++;
    vary_words(F->base.objects, f.objects, &F->v_obj);
    vary_words(F->base.trav, f.trav, &F->v_trav);
    vary_words(F->base.strav, f.strav, &F->v_strav);
    vary_words(F->base.leaves, f.leaves, &F->v_leaf);
    vary_words(F->base.lights, f.lights, &F->v_light);
  }
  // A family of ONE scene gets no family program: the scene's own program (every word a constant, the
  // tables in the constant address space) is the better code -- globes.scene as a family of one
  // spilled to 1 392 B/lane of scratch (its own program: 560) -- so its own program is compiled now.
  Requested all;
  std::vector<size_t> first(fams.size());
  for (size_t fi = 0; fi < fams.size(); ++fi) {
    auto& F = fams[fi];
    SpecProgram p = spec_flags(F->base, 1);        // mode / clamp form / size limits of the class
    if (!p.fits) return not_specialised(F->base, true);
    p.src = F->src = spec_source(F->base, F->members > 1 ? F.get() : nullptr);
    first[fi] = all.jobs.size();
    all.add(p, SPEC_SET_SCENE);
    if (F->members == 1) all.add(p, SPEC_SET_LEAN);  // (a family program holds none)
    F->jobs.assign(all.jobs.begin() + first[fi], all.jobs.end());
  }
  // every class's programs, compiled by the pool in parallel; the families whose programs compiled and
  // passed the guard are registered, the others not (their scenes then compile their own programs)
  double ms = 0.0;
  std::string first_err;
  std::vector<char> good(fams.size(), 0);
  for (size_t fi = 0; fi < fams.size(); ++fi) {
    bool ok = true;
    for (size_t i = first[fi]; i < first[fi] + fams[fi]->jobs.size(); ++i) {
      job_wait(all.jobs[i].get(), -1.0);
      if (all.jobs[i]->state.load() != SPEC_DONE) {
        ok = false;
        if (first_err.empty())
          first_err = "family of " + std::to_string(fams[fi]->members) + " scenes: " + job_error(*all.jobs[i]);
      } else if (!all.was_done[i]) {
        ms = std::max(ms, all.jobs[i]->code.compile_ms);
      }
    }
    good[fi] = ok;
  }
  {
    std::lock_guard<std::mutex> lk(g_family_mu);
    for (size_t fi = 0; fi < fams.size(); ++fi)
      if (good[fi]) (fams[fi]->members > 1 ? g_families : g_singles).push_back(fams[fi]);   // singles: their own program resident
  }
  if (compile_ms) *compile_ms = ms;
  if (!first_err.empty()) return fail(RT_ERR_UNSUPPORTED, "%s", first_err.c_str());
  return RT_OK;
}

// rt_spec_family_clear (include/rt_abi.h): forget every registered family (loaded modules stay)
extern "C" int rt_spec_family_clear(void) {
  std::vector<std::shared_ptr<SpecFamily>> old, old1;
  {
    std::lock_guard<std::mutex> lk(g_family_mu);
    old.swap(g_families);
    old1.swap(g_singles);
  }
  return RT_OK;                                    // `old` drops the families' interest in their programs
}
