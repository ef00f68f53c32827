"""The host side of the batched ray paths (rt_ray_paths_offsets, rt_ray_paths), without a GPU: the scan's partition and
the segment rule (tinyraytracerinrust_amd/csrc/paths_plan.h, pure host code) in a stand-alone program built with the
address and undefined-behaviour sanitizers, the way tests/test_launch_plan.py tests launch_plan.h; the two names in
the header, the binding and INTEGRATION.md's Rust block; the command line's refusals before any GPU is touched."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAMES = ("rt_ray_paths_offsets", "rt_ray_paths")
HARNESS = r"""
#include "paths_plan.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace rt;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)

// the three steps on the host, partitioned exactly as the plan says: block sums, ONE pass over them in rounds of
// RT_SCAN_BLOCK with a carry, then every block's own scan plus its scanned sum
static std::vector<uint64_t> scan_by_plan(const std::vector<uint32_t>& c) {
  const uint64_t n = c.size();
  const ScanPlan p = plan_scan(n);
  std::vector<uint64_t> off(n + 1, ~0ull), sums;
  if (p.status != ScanPlan::OK) { off[0] = 0; return off; }
  if (p.two_level) {
    sums.assign((size_t)p.n_blocks + 1, 0);
    CHECK(p.sums_bytes == sums.size() * 8);
    for (uint32_t b = 0; b < p.n_blocks; ++b) {
      const uint32_t len = b + 1 == p.n_blocks ? p.last_block : RT_SCAN_BLOCK;
      for (uint32_t k = 0; k < len; ++k) sums[b] += c[(size_t)b * RT_SCAN_BLOCK + k];
    }
    uint64_t carry = 0;
    uint32_t rounds = 0;
    for (uint32_t r0 = 0; r0 < p.n_blocks; r0 += RT_SCAN_BLOCK, ++rounds)
      for (uint32_t k = r0; k < p.n_blocks && k < r0 + RT_SCAN_BLOCK; ++k) { const uint64_t s = sums[k]; sums[k] = carry; carry += s; }
    sums[p.n_blocks] = carry;
    CHECK(rounds == p.top_rounds);
  }
  for (uint32_t b = 0; b < p.n_blocks; ++b) {
    const uint32_t len = b + 1 == p.n_blocks ? p.last_block : RT_SCAN_BLOCK;
    uint64_t at = p.two_level ? sums[b] : 0;
    for (uint32_t k = 0; k < len; ++k) { off[(size_t)b * RT_SCAN_BLOCK + k] = at; at += c[(size_t)b * RT_SCAN_BLOCK + k]; }
    if (b + 1 == p.n_blocks) off[n] = at;
  }
  return off;
}

static void plan() {
  CHECK(RT_SCAN_BLOCK == RT_SCAN_THREADS * RT_SCAN_ITEMS && RT_SCAN_BLOCK == 1024);
  CHECK(RT_SCAN_MAX_N == (1ull << 26));
  ScanPlan p = plan_scan(0);
  CHECK(p.status == ScanPlan::NOTHING && p.n_blocks == 0);
  p = plan_scan(1);
  CHECK(p.status == ScanPlan::OK && p.n_blocks == 1 && p.last_block == 1 && !p.two_level && p.top_rounds == 0 && p.sums_bytes == 0);
  p = plan_scan(RT_SCAN_BLOCK - 1);
  CHECK(p.n_blocks == 1 && p.last_block == RT_SCAN_BLOCK - 1 && !p.two_level);
  p = plan_scan(RT_SCAN_BLOCK);                                  // one full block: still the single-workgroup path
  CHECK(p.n_blocks == 1 && p.last_block == RT_SCAN_BLOCK && !p.two_level && p.sums_bytes == 0);
  p = plan_scan(RT_SCAN_BLOCK + 1);
  CHECK(p.n_blocks == 2 && p.last_block == 1 && p.two_level && p.top_rounds == 1 && p.sums_bytes == 24);
  p = plan_scan(4116);                                           // the GPU tests' sample count
  CHECK(p.n_blocks == 5 && p.last_block == 20 && p.two_level && p.top_rounds == 1);
  p = plan_scan(129600);                                         // a 4K frame's centres at step 8
  CHECK(p.n_blocks == 127 && p.last_block == 576 && p.top_rounds == 1);
  p = plan_scan((uint64_t)RT_SCAN_BLOCK * RT_SCAN_BLOCK);        // the top workgroup's first round, full
  CHECK(p.n_blocks == RT_SCAN_BLOCK && p.last_block == RT_SCAN_BLOCK && p.top_rounds == 1);
  p = plan_scan((uint64_t)RT_SCAN_BLOCK * RT_SCAN_BLOCK + 1);
  CHECK(p.n_blocks == RT_SCAN_BLOCK + 1 && p.last_block == 1 && p.top_rounds == 2);
  p = plan_scan(RT_SCAN_MAX_N);                                  // the bound the second level serves
  CHECK(p.status == ScanPlan::OK && p.n_blocks == RT_SCAN_TOP_MAX && p.last_block == RT_SCAN_BLOCK && p.top_rounds == 64);
  p = plan_scan(RT_SCAN_MAX_N + 1);                              // ... and the first n past it
  CHECK(p.status == ScanPlan::TOO_MANY);
  CHECK(plan_scan(~0ull).status == ScanPlan::TOO_MANY);
  for (uint64_t n = 1; n <= 5 * RT_SCAN_BLOCK + 7; ++n) {        // every n over several blocks: the blocks tile [0, n)
    p = plan_scan(n);
    CHECK(p.status == ScanPlan::OK && p.last_block >= 1 && p.last_block <= RT_SCAN_BLOCK);
    CHECK((uint64_t)(p.n_blocks - 1) * RT_SCAN_BLOCK + p.last_block == n);
    CHECK(p.two_level == (n > RT_SCAN_BLOCK));
  }
  printf("plan: %d failures\n", fails);
}

static void scan() {
  const uint64_t sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4116, 5 * 1024 + 7,
                            (uint64_t)RT_SCAN_BLOCK * RT_SCAN_BLOCK + 1500};   // the last: two rounds of the top workgroup
  uint32_t seed = 12345u;
  for (uint64_t n : sizes) {
    std::vector<uint32_t> c((size_t)n);
    for (auto& v : c) { seed = seed * 1664525u + 1013904223u; v = 1 + (seed >> 24) % 34; }   // 1..34 rays, as the fractal
    if (n > 100) c[n - 1] = c[n / 2] = (1u << 17) - 1;           // the most rays a sample can trace at depth 16
    const std::vector<uint64_t> off = scan_by_plan(c);
    uint64_t at = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n; ++i) { ok = ok && off[(size_t)i] == at; at += c[(size_t)i]; }
    CHECK(ok && off[(size_t)n] == at);
  }
  { // sums past 32 bits: every sample at the most rays
    std::vector<uint32_t> c(40000, (1u << 17) - 1);
    const std::vector<uint64_t> off = scan_by_plan(c);
    CHECK(off[40000] == 40000ull * ((1u << 17) - 1) && off[40000] > 0xffffffffull && off[39999] == 39999ull * ((1u << 17) - 1));
  }
  CHECK(scan_by_plan({})[0] == 0);
  printf("scan: %d failures\n", fails);
}

static void segments() {
  PathSegment s = path_segment(10, 14, 100);
  CHECK(s.begin == 10 && s.len == 4);
  s = path_segment(10, 10, 100);  CHECK(s.len == 0);
  s = path_segment(96, 104, 100); CHECK(s.begin == 96 && s.len == 4);      // cut to the buffer
  s = path_segment(100, 104, 100); CHECK(s.len == 0);                      // begins at the end: nothing fits
  s = path_segment(101, 104, 100); CHECK(s.begin == 0 && s.len == 0);      // begins past the end: the empty segment
  s = path_segment(14, 10, 100);  CHECK(s.begin == 0 && s.len == 0);       // decreasing offsets: the empty segment
  s = path_segment(0, ~0ull, 0);  CHECK(s.len == 0);
  s = path_segment(0, ~0ull, ~0ull); CHECK(s.len == RT_PATHS_MAX_RECORDS);  // a length always fits BufRec's int
  const uint64_t edge[] = {0, 1, 2, 99, 100, 101, 0x7fffffffull, 0x80000000ull, 0xffffffffull, 0x100000000ull, ~0ull - 1, ~0ull};
  for (uint64_t o0 : edge) for (uint64_t o1 : edge) for (uint64_t cap : edge) {   // whatever the offsets: inside the buffer
    s = path_segment(o0, o1, cap);
    CHECK(s.begin <= cap && s.len <= cap - s.begin && s.len <= RT_PATHS_MAX_RECORDS);
    if (s.len) CHECK(s.begin == o0 && s.begin + s.len <= o1);
  }
  printf("segments: %d failures\n", fails);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (!strcmp(argv[1], "plan")) plan();
  else if (!strcmp(argv[1], "scan")) scan();
  else if (!strcmp(argv[1], "segments")) segments();
  else return 2;
  return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which("g++"), "the library's own host compiler"
    d = tmp_path_factory.mktemp("paths_plan")
    (d / "h.cpp").write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-Wall", "-Wextra", f"-I{ROOT / 'tinyraytracerinrust_amd' / 'csrc'}", str(d / "h.cpp"),
                        "-o", str(d / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return d / "h"


def run(harness, section):
    r = subprocess.run([str(harness), section], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and f"{section}: 0 failures" in r.stdout


def test_scan_plan_cases(harness):
    """n = 0, 1, one block -1 / exact / +1, several blocks and a remainder, the top workgroup's second round, the bound
    the second level serves and the first n past it."""
    run(harness, "plan")


def test_scan_by_the_plan_is_the_prefix_sum(harness):
    """The three steps carried out on the host, partitioned as the plan says, equal the running sum -- sizes round a
    wave, a workgroup and a block, two rounds of the top workgroup, sums past 32 bits."""
    run(harness, "scan")


def test_segments_stay_inside_the_buffer(harness):
    """The segment rule the fill kernel shares: cut to the buffer, empty for decreasing or out-of-range offsets, and
    for every combination of edge values inside [0, cap)."""
    run(harness, "segments")


# ---------------------------------------------------------------- the two names
def test_library_exports_the_two_symbols():
    import tinyraytracerinrust_amd as T
    lib = T.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rt_abi_version() == 1


def test_header_binding_and_rust_block_agree():
    from tinyraytracerinrust_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rt_abi.h").read_text(), flags=re.S)
    doc = (ROOT / "INTEGRATION.md").read_text()
    block = re.findall(r'extern "C" \{(.*?)\n\}', doc, flags=re.S)[0]
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
        assert m, name
        arity = m.group(1).count(",") + 1
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity, name
        r = re.search(r"pub fn " + name + r"\s*\((.*?)\)\s*->\s*c_int;", block, flags=re.S)
        assert r, name
        assert re.sub(r"//[^\n]*", "", r.group(1)).strip().rstrip(",").count(",") + 1 == arity, name
    assert len(_lib.SIGNATURES["rt_ray_paths_offsets"][1]) == 7 and len(_lib.SIGNATURES["rt_ray_paths"][1]) == 9
    for doc_name in ("README.md", "DESIGN.md"):
        text = (ROOT / doc_name).read_text()
        assert all(name in text for name in NAMES), doc_name


def test_null_context_is_refused():
    import tinyraytracerinrust_amd as T
    lib = T.lib()
    xy = (ctypes.c_double * 2)(1.0, 2.0)
    offsets = (ctypes.c_uint64 * 2)(7, 7)
    total = ctypes.c_uint64(7)
    rec = (ctypes.c_uint8 * 160)()
    assert lib.rt_ray_paths_offsets(None, xy, 1, -1, offsets, ctypes.byref(total), None) == -1
    assert lib.rt_ray_paths(None, xy, 1, -1, offsets, rec, 1, None, None) == -1
    assert list(offsets) == [7, 7] and total.value == 7


def test_record_dtype_is_ten_16_byte_chunks():
    from tinyraytracerinrust_amd.raytracer import RAY_RECORD_DTYPE
    assert RAY_RECORD_DTYPE.itemsize == 160
    assert RAY_RECORD_DTYPE.fields["pad"][1] == 20          # the word of chunk 1 the gather stores as 0


# ---------------------------------------------------------------- the command line
def test_parser_accepts_ray_paths():
    from tinyraytracerinrust_amd.__main__ import _parse
    a = _parse(["render", "x.scene", "--ray-paths", "p.npz"])
    assert a.ray_paths == "p.npz" and a.ray_paths_step == 8
    assert _parse(["render", "x.scene", "--ray-paths", "p.npz", "--ray-paths-step", "3"]).ray_paths_step == 3
    assert _parse(["render", "x.scene"]).ray_paths is None


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--camera", "anaglyph", "--eye-distance", "6.5"],
                                   ["--camera", "stereoscopic", "--eye-distance", "6.5"], ["--ray-paths-step", "0"]])
def test_parser_refuses_ray_paths(extra, capsys):
    from tinyraytracerinrust_amd.__main__ import _parse
    with pytest.raises(SystemExit) as e:
        _parse(["render", "x.scene", "--ray-paths", "p.npz"] + extra)
    assert e.value.code != 0
    assert "--ray-paths" in capsys.readouterr().err


def test_sample_grid_is_every_nth_pixel_centre_row_major():
    from tinyraytracerinrust_amd.__main__ import ray_paths_samples
    xy = ray_paths_samples(10, 7, 4)
    assert xy.dtype == np.float64
    assert xy.tolist() == [[0, 0], [4, 0], [8, 0], [0, 4], [4, 4], [8, 4]]
    assert ray_paths_samples(3840, 2160, 8).shape == (129600, 2)
    assert ray_paths_samples(5, 5, 1).shape == (25, 2)
