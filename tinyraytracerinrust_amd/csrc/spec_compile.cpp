// spec_compile.cpp -- the compiler of the scene-specialised programs (spec.h): hipRTC, the code object's
// metadata and the resource guard.  No context, no HIP runtime: a text in, a code object out.
//
// Guards: only the ROCm installation's hipRTC compiles (loaded into a link-map namespace of its own, see
// rtc()), and a code object whose resource use exceeds the known-good bound (VGPRs, scratch per lane,
// from the code object's metadata) is refused -- the context then keeps the generic kernels and
// rt_ctx_kernel_info says why.
#include <dlfcn.h>
#include <hip/hiprtc.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>

#include "spec.h"

namespace {

// The device headers as text: spec_headers[], {name, text} pairs in the order of the Makefile's SPEC_HDRS
// (build/spec_headers.inc: raw string literals made by the Makefile).
#include "spec_headers.inc"

// The hipRTC the programs compile with: the ROCm installation's own (ROCM_PATH, default /opt/rocm),
// loaded into a link-map namespace of its own (dlmopen) with the code-object manager (comgr) it
// loads.  In a process that imported PyTorch first, the plain libhiprtc.so.7 / libamd_comgr.so.3
// resolve to the copies PyTorch bundles (ROCm 7.0, LLVM 20), whose codegen of the scene-family
// program came out 3.8x larger (128 VGPRs, 1.4 KB/lane of scratch) and 19x slower than this
// ROCm's (LLVM 22; profiles/r05v_family_compilers.txt).  If the namespace cannot be made, the
// process's hipRTC is used and the kernel info says so.
struct Rtc : rt::SpecCompiler {
  hiprtcResult (*create)(hiprtcProgram*, const char*, const char*, int, const char* const*, const char* const*);
  hiprtcResult (*compile)(hiprtcProgram, int, const char* const*);
  hiprtcResult (*log_size)(hiprtcProgram, size_t*);
  hiprtcResult (*log)(hiprtcProgram, char*);
  hiprtcResult (*code_size)(hiprtcProgram, size_t*);
  hiprtcResult (*code)(hiprtcProgram, char*);
  hiprtcResult (*destroy)(hiprtcProgram*);
  const char* (*err)(hiprtcResult);
  hiprtcResult (*version)(int*, int*);
};
const Rtc& rtc() {
  static const Rtc r = [] {
    Rtc x;
    const char* root = getenv("ROCM_PATH");
    const std::string path = std::string(root && *root ? root : "/opt/rocm") + "/lib/libhiprtc.so.7";
    void* h = dlmopen(LM_ID_NEWLM, path.c_str(), RTLD_NOW | RTLD_LOCAL);
    auto sym = [&](const char* n) { return h ? dlsym(h, n) : nullptr; };
    x.rocm = h && sym("hiprtcCreateProgram") && sym("hiprtcCompileProgram") && sym("hiprtcGetCode");
#define RTC_BIND(field, fn) x.field = x.rocm ? (decltype(x.field))sym(#fn) : fn
    RTC_BIND(create, hiprtcCreateProgram);
    RTC_BIND(compile, hiprtcCompileProgram);
    RTC_BIND(log_size, hiprtcGetProgramLogSize);
    RTC_BIND(log, hiprtcGetProgramLog);
    RTC_BIND(code_size, hiprtcGetCodeSize);
    RTC_BIND(code, hiprtcGetCode);
    RTC_BIND(destroy, hiprtcDestroyProgram);
    RTC_BIND(err, hiprtcGetErrorString);
    RTC_BIND(version, hiprtcVersion);
#undef RTC_BIND
    x.origin = x.rocm ? path : std::string("the process's libhiprtc (") + (h ? "symbols missing" : dlerror()) + ")";
    int ma = 0, mi = 0;
    if (x.version && x.version(&ma, &mi) == HIPRTC_SUCCESS) x.origin += " " + std::to_string(ma) + "." + std::to_string(mi);
    x.identity = x.origin;
    if (char* rp = realpath(path.c_str(), nullptr)) {
      struct stat st;
      if (stat(rp, &st) == 0)
        x.identity += std::string(" ") + rp + " " + std::to_string((long long)st.st_size) + " " + std::to_string((long long)st.st_mtime);
      free(rp);
    }
    return x;
  }();
  return r;
}

// Resource guard: the known-good bounds of the specialised kernels (ROCm 7.2's LLVM: the reflection and
// chain megakernels at most 128 VGPRs at 4 waves/SIMD with 528-576 B/lane of scratch; the ray-tree
// megakernel 1 424 B/lane for its pending-reflection stack, the deferred kernel 1 568 B/lane for its
// per-lane hit records).  PyTorch's bundled LLVM 20 built the chain family megakernel with 1.4 KB/lane
// and ran it 19x slower (profiles/r05v_family_compilers.txt): that is what the guard refuses.
#ifndef RT_SPEC_MAX_VGPRS
#define RT_SPEC_MAX_VGPRS 128
#endif
#ifndef RT_SPEC_MAX_SCRATCH_ROWS
#define RT_SPEC_MAX_SCRATCH_ROWS 1024
#endif
#ifndef RT_SPEC_MAX_SCRATCH_DEF
#define RT_SPEC_MAX_SCRATCH_DEF 2048
#endif
#ifndef RT_SPEC_MAX_SCRATCH_TREE
#define RT_SPEC_MAX_SCRATCH_TREE 2048
#endif

// The kernel's resource use from the code object's AMDGPU metadata note (msgpack): the map entry after
// the key string, e.g. ".vgpr_count" -> 128.  One kernel per program, so every key occurs once.
// (hipRTC's -Rpass-analysis=kernel-resource-usage remarks say the same, but emitting them crashed the
// compiler inside its own link-map namespace.)
bool mp_value(const std::vector<char>& b, const char* key, long long* ival, std::string* sval) {
  const size_t n = strlen(key);
  std::string pat;
  if (n < 32) pat += (char)(0xa0 | n);
  else { pat += (char)0xd9; pat += (char)n; }
  pat += key;
  const auto it = std::search(b.begin(), b.end(), pat.begin(), pat.end());
  if (it == b.end()) return false;
  size_t i = (size_t)(it - b.begin()) + pat.size();
  if (i >= b.size()) return false;
  const unsigned char t = (unsigned char)b[i];
  auto be = [&](int bytes) {
    unsigned long long v = 0;
    for (int k = 1; k <= bytes && i + k < b.size(); ++k) v = v << 8 | (unsigned char)b[i + k];
    return v;
  };
  if (sval) {
    size_t len = 0, at = 0;
    if ((t & 0xe0) == 0xa0) { len = t & 0x1f; at = i + 1; }
    else if (t == 0xd9) { len = (size_t)be(1); at = i + 2; }
    else return false;
    if (at + len > b.size()) return false;
    sval->assign(b.data() + at, len);
    return true;
  }
  if (t <= 0x7f) *ival = t;
  else if (t == 0xcc) *ival = (long long)be(1);
  else if (t == 0xcd) *ival = (long long)be(2);
  else if (t == 0xce) *ival = (long long)be(4);
  else if (t == 0xcf) *ival = (long long)be(8);
  else return false;
  return true;
}

// The hipRTC options: the flags the library's own kernels are built with (Makefile HIPFLAGS: -O3, no
// contraction, no fast-math, MachineLICM off).
std::vector<std::string> spec_options() {
  std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                                   "-mllvm", "-disable-machine-licm"};
#ifdef RT_DIAG_ENV
  // diagnostic builds: RT_SPEC_OPTS appends options (space-separated) for compiler A/B runs
  if (const char* e = getenv("RT_SPEC_OPTS")) {
    std::string s(e), w;
    for (size_t i = 0; i <= s.size(); ++i)
      if (i == s.size() || s[i] == ' ') { if (!w.empty()) opts.push_back(w); w.clear(); } else w += s[i];
  }
#endif
  return opts;
}

}  // namespace

namespace rt {

const SpecCompiler& spec_compiler() { return rtc(); }

void code_resources(SpecCode* c) {
  long long v = -1;
  c->vgprs = mp_value(c->code, ".vgpr_count", &v, nullptr) ? (int)v : -1;
  c->sgprs = mp_value(c->code, ".sgpr_count", &v, nullptr) ? (int)v : -1;
  c->scratch = mp_value(c->code, ".private_segment_fixed_size", &v, nullptr) ? (int)v : -1;
  c->vspill = mp_value(c->code, ".vgpr_spill_count", &v, nullptr) ? (int)v : -1;
  c->occupancy = c->vgprs > 0 ? std::min(8, 512 / ((c->vgprs + 7) / 8 * 8)) : -1;   // VGPR-limited waves/SIMD
  std::string name;
  c->name = mp_value(c->code, ".name", nullptr, &name) ? name : "";
}

// The disk-cache identity of a code object: the compiler's (rtc().identity) plus a hash of everything
// else the object depends on besides the program text -- the device headers this library embeds (the
// text only #includes them) and the compile options.  A rebuild that changes a header (a record layout,
// a kernel argument) changes the identity, so an entry written by another build is never read.
std::string spec_build_identity() {
  std::string key;
  for (const auto& h : spec_headers) {
    key += h.text;
    key += '\0';
  }
  for (const std::string& o : spec_options()) {
    key += o;
    key += '\0';
  }
  char buf[40];
  snprintf(buf, sizeof buf, " build %016llx", (unsigned long long)fnv1a(key));
  return rtc().identity + buf;
}

// hipRTC: the program (with the device headers as named headers), spec_options(), and the resource use
// the guard reads from the code object.
int spec_compile(const std::string& src, SpecCode* out, std::string* err) {
  std::vector<const char*> headers, names;
  for (const auto& h : spec_headers) {
    headers.push_back(h.text);
    names.push_back(h.name);
  }
  hiprtcProgram prog;
  const Rtc& R = rtc();
  if (R.create(&prog, src.c_str(), "rt_spec.hip", (int)headers.size(), headers.data(), names.data()) != HIPRTC_SUCCESS) {
    *err = "hiprtcCreateProgram failed";
    return RT_ERR_DEVICE;
  }
  const std::vector<std::string> ostr = spec_options();
  std::vector<const char*> opts;
  for (const std::string& x : ostr) opts.push_back(x.c_str());
  const auto t0 = std::chrono::steady_clock::now();
  const hiprtcResult r = R.compile(prog, (int)opts.size(), opts.data());
  out->compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  size_t n = 0;
  R.log_size(prog, &n);
  std::string log(n + 1, '\0');
  if (n) R.log(prog, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    R.destroy(&prog);
    char buf[2300];
    snprintf(buf, sizeof buf, "hipRTC compile of the specialised kernels failed: %s\n%.2000s", R.err(r), log.c_str());
    *err = buf;
    return RT_ERR_DEVICE;
  }
  n = 0;
  R.code_size(prog, &n);
  out->code.resize(n);
  R.code(prog, out->code.data());
  R.destroy(&prog);
  code_resources(out);
#ifdef RT_DIAG_ENV
  if (const char* dir = getenv("RT_SPEC_DUMP_DIR")) {     // diagnostic builds: the code object and its text
    char path[512];
    snprintf(path, sizeof path, "%s/spec_%016llx.co", dir, (unsigned long long)fnv1a(src));
    if (FILE* fo = fopen(path, "wb")) { fwrite(out->code.data(), 1, n, fo); fclose(fo); }
    snprintf(path, sizeof path, "%s/spec_%016llx.hip", dir, (unsigned long long)fnv1a(src));
    if (FILE* fo = fopen(path, "wb")) { fwrite(src.data(), 1, src.size(), fo); fclose(fo); }
  }
#endif
  return RT_OK;
}

int spec_guard(const SpecCode& c, SpecBound bound, std::string* err) {
  const int max_scratch = bound == SPEC_BOUND_DEFERRED ? RT_SPEC_MAX_SCRATCH_DEF
                          : bound == SPEC_BOUND_TREE   ? RT_SPEC_MAX_SCRATCH_TREE
                                                       : RT_SPEC_MAX_SCRATCH_ROWS;
  if (c.name.empty() || c.vgprs < 0 || c.scratch < 0) {
    *err = "resource guard: the code object's metadata holds no resource usage for the kernel";
    return RT_ERR_UNSUPPORTED;
  }
  if (c.vgprs > RT_SPEC_MAX_VGPRS || c.scratch > max_scratch) {
    char buf[256];
    snprintf(buf, sizeof buf, "resource guard: %s uses %d VGPRs and %d B/lane of scratch (bounds %d / %d)", c.name.c_str(),
             c.vgprs, c.scratch, RT_SPEC_MAX_VGPRS, max_scratch);
    *err = buf;
    return RT_ERR_UNSUPPORTED;
  }
  return RT_OK;
}

}  // namespace rt

// rt_spec_compiler_info (include/rt_abi.h): which hipRTC the programs compile with
extern "C" int rt_spec_compiler_info(char* buf, size_t cap, int32_t* rocm) {
  if (rocm) *rocm = rtc().rocm ? 1 : 0;
  if (buf && cap > 0) snprintf(buf, cap, "%s", rt::spec_build_identity().c_str());
  return RT_OK;
}
