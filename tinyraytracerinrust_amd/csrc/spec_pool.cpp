// spec_pool.cpp -- the job table of the scene-specialised programs (spec.h), the pool of library threads
// that compiles them, and the process and on-disk caches.  No context, no HIP runtime: it sees a program's
// text and the scratch bound its code object is held to.
//
//   * a request returns at once: a small pool of library threads compiles the program (or finds it in the
//     process cache / the on-disk cache) while the caller renders with the generic kernels;
//   * a program is keyed by its FULL text (the process cache compares the text, the disk cache the
//     text and the compiler's identity), never by a hash alone.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <map>
#include <thread>

#include "spec.h"

namespace {

using namespace rt;

// At most this many compiles at once (hipRTC / LLVM: seconds and hundreds of MB each).
constexpr size_t RT_SPEC_WORKERS_MAX = 4;
// Completed programs the process keeps when nobody holds them (LRU beyond this many jobs).
constexpr size_t RT_SPEC_CACHE_JOBS = 64;

std::mutex g_spec_mu;                  // the job table
struct SpecState {                     // under g_spec_mu; never destroyed (workers may outlive exit's destructors)
  std::map<std::string, std::shared_ptr<SpecJob>> jobs;   // by full program text
  uint64_t clock = 0;
  std::deque<std::shared_ptr<SpecJob>> queue;
  std::vector<std::thread> workers;
  std::condition_variable qcv;
  bool stop = false;
  std::string disk_dir;                // rt_spec_cache_dir: "" = no on-disk cache
};
SpecState& sst() {
  static SpecState* p = new SpecState;
  return *p;
}

void job_finish(SpecJob* j, int state) {
  {
    std::lock_guard<std::mutex> lk(j->mu);
    j->state = state;
  }
  j->cv.notify_all();
}

// A token of interest in job j: a shared_ptr to the job whose deleter drops the interest again.
std::shared_ptr<SpecJob> job_token(const std::shared_ptr<SpecJob>& j) {
  j->interest++;
  return std::shared_ptr<SpecJob>(j.get(), [j](SpecJob*) { j->interest--; });
}

// On-disk cache entry: "RTSPEC03\n", then length-prefixed (u64) identity (spec_build_identity), program
// text, kernel name and code object.  A hit must match identity AND text; the resource numbers the guard
// checks are read from the code object itself (code_resources), never from the file.
void put_blob(std::string& f, const void* p, uint64_t n) {
  f.append((const char*)&n, 8);
  f.append((const char*)p, n);
}
bool get_blob(const std::vector<char>& f, size_t* at, std::string* s) {
  uint64_t n = 0;
  if (*at + 8 > f.size()) return false;
  memcpy(&n, f.data() + *at, 8);
  *at += 8;
  if (n > f.size() - *at) return false;
  s->assign(f.data() + *at, n);
  *at += n;
  return true;
}
std::string disk_path(const std::string& dir, const std::string& identity, const std::string& text) {
  char buf[64];
  snprintf(buf, sizeof buf, "/spec_%016llx.rtco", (unsigned long long)fnv1a(identity + '\0' + text));
  return dir + buf;
}
bool disk_read(const std::string& path, const std::string& identity, const std::string& text, SpecCode* out) {
  FILE* fi = fopen(path.c_str(), "rb");
  if (!fi) return false;
  std::vector<char> f;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fi)) > 0) f.insert(f.end(), buf, buf + n);
  fclose(fi);
  static const char magic[] = "RTSPEC03\n";
  if (f.size() < 9 || memcmp(f.data(), magic, 9) != 0) return false;
  size_t at = 9;
  std::string id, tx, name, code;
  if (!get_blob(f, &at, &id) || id != identity || !get_blob(f, &at, &tx) || tx != text || !get_blob(f, &at, &name) ||
      !get_blob(f, &at, &code) || at != f.size())
    return false;
  out->code.assign(code.begin(), code.end());
  code_resources(out);                                    // name and resources from the code object's metadata
  if (out->name != name) return false;
  out->compile_ms = 0.0;
  out->from_disk = true;
  return true;
}
void disk_write(const std::string& dir, const std::string& path, const std::string& identity, const std::string& text,
                const SpecCode& c) {
  for (size_t i = 1; i <= dir.size(); ++i)              // mkdir -p
    if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
  std::string f("RTSPEC03\n");
  put_blob(f, identity.data(), identity.size());
  put_blob(f, text.data(), text.size());
  put_blob(f, c.name.data(), c.name.size());
  put_blob(f, c.code.data(), c.code.size());
  char tmp[64];
  snprintf(tmp, sizeof tmp, ".tmp.%d.%llx", (int)getpid(), (unsigned long long)std::hash<std::thread::id>()(std::this_thread::get_id()));
  const std::string tp = path + tmp;
  FILE* fo = fopen(tp.c_str(), "wb");
  if (!fo) return;                                        // the cache is an optimisation: no error
  const bool ok = fwrite(f.data(), 1, f.size(), fo) == f.size();
  if (fclose(fo) == 0 && ok) (void)rename(tp.c_str(), path.c_str());
  else (void)unlink(tp.c_str());
}

// The code object of one program: the on-disk cache, else hipRTC; then the resource guard.
int spec_obtain(const std::string& text, SpecBound bound, SpecCode* out, std::string* err) {
  const SpecCompiler& R = spec_compiler();
  if (!R.rocm) {
    *err = "hipRTC guard: the ROCm installation's libhiprtc could not be loaded into a namespace of its own (" + R.origin +
           "); another hipRTC in the process (PyTorch bundles an older LLVM) is not used";
    return RT_ERR_UNSUPPORTED;
  }
  std::string dir;
  {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    dir = sst().disk_dir;
  }
  const std::string ident = dir.empty() ? "" : spec_build_identity();
  const std::string path = dir.empty() ? "" : disk_path(dir, ident, text);
  if (!path.empty() && disk_read(path, ident, text, out)) return spec_guard(*out, bound, err);
  int rc = spec_compile(text, out, err);
  if (!rc) rc = spec_guard(*out, bound, err);
  if (!rc && !path.empty()) disk_write(dir, path, ident, text, *out);
  return rc;
}

void spec_worker() {
  SpecState& S = sst();
  for (;;) {
    std::shared_ptr<SpecJob> j;
    {
      std::unique_lock<std::mutex> lk(g_spec_mu);
      S.qcv.wait(lk, [&] { return S.stop || !S.queue.empty(); });
      if (S.queue.empty()) return;                        // shut down
      j = S.queue.front();
      S.queue.pop_front();
      if (j->interest.load() == 0) {                      // nobody renders this program any more
        auto it = S.jobs.find(j->text);
        if (it != S.jobs.end() && it->second == j) S.jobs.erase(it);
        job_finish(j.get(), SPEC_CANCELLED);
        continue;
      }
      j->state = SPEC_RUNNING;
    }
    std::string err;
    const int rc = spec_obtain(j->text, j->bound, &j->code, &err);
    if (rc) j->error = err;
    job_finish(j.get(), rc ? SPEC_FAILED : SPEC_DONE);
  }
}

}  // namespace

namespace rt {

uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ull; }
  return h;
}

bool job_finished(const SpecJob* j) {
  const int s = j->state.load();
  return s == SPEC_DONE || s == SPEC_FAILED || s == SPEC_CANCELLED;
}

bool job_wait(SpecJob* j, double timeout_ms) {
  std::unique_lock<std::mutex> lk(j->mu);
  if (timeout_ms < 0) {
    j->cv.wait(lk, [&] { return job_finished(j); });
    return true;
  }
  return j->cv.wait_for(lk, std::chrono::duration<double, std::milli>(timeout_ms), [&] { return job_finished(j); });
}

bool jobs_wait(const std::vector<std::shared_ptr<SpecJob>>& jobs, double timeout_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  for (const auto& j : jobs) {
    double left = -1.0;
    if (timeout_ms >= 0)
      left = std::max(0.0, timeout_ms - std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (!job_wait(j.get(), left)) return false;
  }
  return true;
}

std::string job_error(const SpecJob& j) {
  const int s = j.state.load();
  return s == SPEC_DONE ? "" : s == SPEC_CANCELLED ? "compile cancelled (rt_spec_shutdown)" : j.error;
}

std::shared_ptr<SpecJob> spec_request(const std::string& text, SpecBound bound, bool retry, bool* was_done) {
  std::lock_guard<std::mutex> lk(g_spec_mu);
  SpecState& S = sst();
  auto it = S.jobs.find(text);
  if (it != S.jobs.end()) {
    const std::shared_ptr<SpecJob> j = it->second;
    const int st = j->state.load();
    if (st != SPEC_CANCELLED && !(retry && st == SPEC_FAILED)) {
      j->last_use = ++S.clock;
      if (was_done) *was_done = st == SPEC_DONE;
      return job_token(j);
    }
    S.jobs.erase(it);
  }
  if (was_done) *was_done = false;
  auto j = std::make_shared<SpecJob>();
  j->text = text;
  j->bound = bound;
  j->last_use = ++S.clock;
  if (S.jobs.size() >= RT_SPEC_CACHE_JOBS) {              // evict the least recently used finished jobs nobody holds
    std::vector<std::pair<uint64_t, std::string>> idle;
    for (auto& kv : S.jobs)
      if (kv.second->interest.load() == 0 && job_finished(kv.second.get())) idle.push_back({kv.second->last_use, kv.first});
    std::sort(idle.begin(), idle.end());
    for (size_t i = 0; i < idle.size() && S.jobs.size() >= RT_SPEC_CACHE_JOBS; ++i) S.jobs.erase(idle[i].second);
  }
  S.jobs.emplace(text, j);
  if (S.stop) {
    j->error = "the specialisation pool is shut down (rt_spec_shutdown)";
    j->state = SPEC_FAILED;
    return job_token(j);
  }
  S.queue.push_back(j);
  const size_t want = std::min<size_t>(RT_SPEC_WORKERS_MAX, std::max(1u, std::thread::hardware_concurrency()));
  if (S.workers.size() < want) {
    // A host that exits while a compile runs would tear down hipRTC / LLVM under a live worker: the
    // first worker registers rt_spec_shutdown at exit (it waits for running compiles, cancels queued
    // ones), so every host is covered, not only the Python wrapper (which also calls it).
    static std::once_flag at_exit;
    std::call_once(at_exit, [] { atexit(rt_spec_shutdown); });
    S.workers.emplace_back(spec_worker);
  }
  S.qcv.notify_one();
  return job_token(j);
}

}  // namespace rt

// rt_spec_cache_dir (include/rt_abi.h): the on-disk code-object cache ("" or NULL: none)
extern "C" int rt_spec_cache_dir(const char* dir) {
  std::lock_guard<std::mutex> lk(g_spec_mu);
  sst().disk_dir = dir ? dir : "";
  while (sst().disk_dir.size() > 1 && sst().disk_dir.back() == '/') sst().disk_dir.pop_back();
  return RT_OK;
}

// rt_spec_shutdown (include/rt_abi.h): cancel queued compiles, wait for running ones, stop the pool
extern "C" void rt_spec_shutdown(void) {
  std::vector<std::thread> th;
  {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    SpecState& S = sst();
    S.stop = true;
    for (auto& j : S.queue) {
      auto it = S.jobs.find(j->text);
      if (it != S.jobs.end() && it->second == j) S.jobs.erase(it);
      job_finish(j.get(), SPEC_CANCELLED);
    }
    S.queue.clear();
    th.swap(S.workers);
    S.qcv.notify_all();
  }
  for (auto& t : th) t.join();
}
