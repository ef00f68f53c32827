"""RT_OPT_TRACED_MASKS 3 on the CPU (launch_plan.h plan_row_launch): which launches take a traced record table,
and which form of it -- the one whose entries with a pixel on a boxed object are traced too
(LaunchPlan::traced_objects: values 1 and 3) or the floor-only one (value 2).  The words and the pixels are
checked on the GPU (tests/test_gpu_traced_object_tiles.py)."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "tinyraytracerinrust_amd" / "csrc"

HARNESS = r"""
#include "launch_plan.h"
#include <cstdio>
using namespace rt;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)
// globes-like: reflection-only, the single-scene program loaded with every kind, the library's own choices, an
// ordered launch whose calibration found it throughput-bound, past the gate
static LaunchFacts base(int traced) {
  LaunchFacts f = {};
  f.colour_fast = true; f.n_lights = 2; f.n_objects = 6;
  f.kernel_opt = RT_KERNEL_AUTO; f.tile_order = true; f.tile_masks = 1; f.tile_records = f.sky_fill = f.fast_clamp = true;
  f.sky_ok = f.masks_ok = true;
  f.max_depth = 10; f.n_tiles = 129600; f.slot = LaunchFacts::ORDERED; f.masks_pay = true;
  f.sh_trcap = 128; f.split_tile_mask = 0xFFFFFu; f.pool_byte_index = true;
  f.loaded = true; f.mode = RT_MODE_REFL; f.fc = true;
  for (int k = 0; k < SPEC_KINDS; ++k) f.has[k] = true;
  f.has_rows_ordered = true;
  f.lean_tiles = f.has_lean = true;
  f.traced_masks = traced; f.has_check = true; f.launches_since_upload = RT_TRACED_MIN_LAUNCHES;
  return f;
}
int main() {
  LaunchPlan pz = {};
  CHECK(!pz.traced && !pz.traced_objects);                         // the new member defaults to off
  LaunchFacts f;
  LaunchPlan p;
  // ---- value 3: every megakernel launch with records, the form with the object entries
  f = base(3);
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects && p.lean && p.records && p.masks && p.sky && p.kind == SPEC_ROWS && p.path == LaunchPlan::MEGA);
  f = base(3); f.launches_since_upload = 0;                        // it does not wait for the gate
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects);
  f = base(3); f.slot = LaunchFacts::NONE; f.tile_masks = 2;       // an unordered launch with masks forced
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects);
  f = base(3); f.masks_pay = false; f.tile_masks = 2;              // a tail-bound order with masks forced
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects);
  f = base(3); f.lean_tiles = false;                               // the lean option is independent
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects && !p.lean);
  // ---- value 2: the same launches, the floor-only form
  f = base(2);
  p = plan_row_launch(f);
  CHECK(p.traced && !p.traced_objects);
  f = base(2); f.launches_since_upload = 0;
  p = plan_row_launch(f);
  CHECK(p.traced && !p.traced_objects);
  // ---- value 1: the value-3 form, only past the gate and where the masks pay
  f = base(1);
  p = plan_row_launch(f);
  CHECK(p.traced && p.traced_objects);
  f = base(1); f.launches_since_upload = RT_TRACED_MIN_LAUNCHES - 1;
  p = plan_row_launch(f);
  CHECK(!p.traced && !p.traced_objects && p.records && p.lean && p.masks);
  f = base(1); f.launches_since_upload = 0;
  p = plan_row_launch(f);
  CHECK(!p.traced && !p.traced_objects);
  f = base(1); f.masks_pay = false; f.tile_masks = 2;
  p = plan_row_launch(f);
  CHECK(!p.traced && !p.traced_objects && p.records);
  f = base(1); f.slot = LaunchFacts::NONE; f.tile_masks = 2;
  p = plan_row_launch(f);
  CHECK(!p.traced && !p.traced_objects && p.records);
  CHECK(RT_TRACED_MIN_LAUNCHES == 8);
  // ---- value 0
  f = base(0);
  p = plan_row_launch(f);
  CHECK(!p.traced && !p.traced_objects && p.records && p.lean);
  // ---- never: depth-0 and calibrating launches, and everything else that takes no traced table
  for (int opt = 1; opt <= 3; ++opt) {
    f = base(opt); f.max_depth = 0;                                // the primary-ray kernel keeps the predicate's words
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects && p.path == LaunchPlan::PRIMARY && p.records);
    f = base(opt); f.slot = LaunchFacts::CALIBRATING; f.tile_masks = 2;
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects && p.records);
    f = base(opt); f.tile_records = false;
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects && p.masks);
    f = base(opt); f.tile_masks = 0;                               // the mask-free megakernel
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects && p.kind == SPEC_ROWS_NOMASK);
    f = base(opt); f.kernel_opt = RT_KERNEL_DEFERRED;
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects);
    f = base(opt); f.kernel_opt = RT_KERNEL_WAVEFRONT;
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects);
    f = base(opt); f.family = true;
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects);
    f = base(opt); f.has_check = false;                            // a program without the pass
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects);
    f = base(opt); f.loaded = false;                               // the generic kernels
    p = plan_row_launch(f);
    CHECK(!p.traced && !p.traced_objects);
  }
  // the decision reads nothing but the facts
  f = base(3);
  CHECK(plan_row_launch(f).traced_objects == plan_row_launch(f).traced_objects);
  printf("%d failures\n", fails);
  return fails != 0;
}
"""


def test_plan_truth_table_for_value_3(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    (tmp_path / "h.cpp").write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", str(tmp_path / "h.cpp"), "-o",
                        str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]


def test_option_setter_takes_0_to_3():
    """The range the setter accepts, read from its source: a context needs a GPU, and the rejection itself is
    exercised there (tests/test_gpu_traced_object_tiles.py)."""
    ctx = (CSRC / "rt_ctx.hip").read_text()
    m = re.search(r"if \(option == RT_OPT_TRACED_MASKS\) \{\s*if \(([^)]*)\) return fail\(RT_ERR_INVALID,", ctx)
    assert m and re.sub(r"\s+", "", m.group(1)) == "value<0||value>3", m and m.group(1)
