"""Traced tile masks (RT_OPT_TRACED_MASKS) on the CPU: when a launch takes a traced record table (launch_plan.h
plan_row_launch), which programs hold the trace pass -- the check kernel with its `mode` argument (spec_text.cpp)
-- and the option's declarations.  The words and the pixels are checked on the GPU (tests/test_gpu_traced_masks.py)."""
import pathlib
import re
import shutil
import subprocess

import pytest

from tests.conftest import SCENES, scene_text

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "tinyraytracerinrust_amd" / "csrc"
FLOOR = "draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))\n"
LIGHT = "append light(<0, 30, -35>, white * 0.5, 100)\n"

HARNESS = r"""
#include "launch_plan.h"
#include <cstdio>
using namespace rt;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)
// globes-like: reflection-only, the single-scene program loaded with every kind, the library's own choices, an
// ordered launch whose calibration found it throughput-bound
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
  LaunchFacts z = {};
  CHECK(z.traced_masks == 0 && !z.has_check);                      // new members default to off
  LaunchPlan pz = {};
  CHECK(!pz.traced);
  // ---- on
  LaunchFacts f = base(1);                                         // option 1: an ordered slot whose masks pay
  LaunchPlan p = plan_row_launch(f);
  CHECK(p.traced && p.lean && p.records && p.masks && p.sky && p.kind == SPEC_ROWS && p.path == LaunchPlan::MEGA);
  f = base(2);                                                     // option 2
  CHECK(plan_row_launch(f).traced);
  f = base(2); f.slot = LaunchFacts::NONE; f.tile_masks = 2;       // option 2: an unordered launch with masks forced
  CHECK(plan_row_launch(f).traced);
  f = base(2); f.masks_pay = false; f.tile_masks = 2;              // option 2: a tail-bound order with masks forced
  CHECK(plan_row_launch(f).traced);
  f = base(2); f.lean_tiles = false;                               // the lean option is independent
  p = plan_row_launch(f);
  CHECK(p.traced && !p.lean);
  // ---- off
  for (int opt = 1; opt <= 2; ++opt) {
    f = base(opt); f.slot = LaunchFacts::CALIBRATING; f.tile_masks = 2;   // a calibrating slot
    p = plan_row_launch(f);
    CHECK(!p.traced && p.records);
    f = base(opt); f.tile_records = false;                         // no records
    p = plan_row_launch(f);
    CHECK(!p.traced && p.masks);
    f = base(opt); f.tile_masks = 0;                               // the mask-free megakernel
    p = plan_row_launch(f);
    CHECK(!p.traced && p.kind == SPEC_ROWS_NOMASK);
    f = base(opt); f.kernel_opt = RT_KERNEL_DEFERRED;              // the deferred path
    p = plan_row_launch(f);
    CHECK(!p.traced && p.path == LaunchPlan::DEFERRED);
    f = base(opt); f.slot_deferred = true;
    CHECK(!plan_row_launch(f).traced);
    f = base(opt); f.kernel_opt = RT_KERNEL_WAVEFRONT;             // the wavefront path
    p = plan_row_launch(f);
    CHECK(!p.traced && p.path == LaunchPlan::WAVEFRONT);
    f = base(opt); f.family = true;                                // a family program
    CHECK(!plan_row_launch(f).traced);
    f = base(opt); f.has_check = false;                            // a program without the pass
    CHECK(!plan_row_launch(f).traced);
    f = base(opt); f.loaded = false;                               // the generic kernels
    CHECK(!plan_row_launch(f).traced);
    f = base(opt); f.max_depth = 0;                                // the primary-ray kernel keeps the predicate's words
    p = plan_row_launch(f);
    CHECK(!p.traced && p.path == LaunchPlan::PRIMARY && p.records);
  }
  f = base(0);                                                     // option 0
  p = plan_row_launch(f);
  CHECK(!p.traced && p.lean && p.records);
  f = base(0); f.tile_masks = 2;
  CHECK(!plan_row_launch(f).traced);
  f = base(1); f.slot = LaunchFacts::NONE; f.tile_masks = 2;       // option 1: an unordered launch, masks forced
  p = plan_row_launch(f);
  CHECK(!p.traced && p.records && p.lean);
  f = base(1); f.masks_pay = false; f.tile_masks = 2;              // option 1: a tail-bound order, masks forced
  p = plan_row_launch(f);
  CHECK(!p.traced && p.records);
  f = base(1); f.launches_since_upload = RT_TRACED_MIN_LAUNCHES - 1;   // option 1: a fresh upload reads the predicate's table
  p = plan_row_launch(f);
  CHECK(!p.traced && p.records && p.lean && p.masks);
  f = base(1); f.launches_since_upload = 0;
  CHECK(!plan_row_launch(f).traced);
  f = base(2); f.launches_since_upload = 0;                        // option 2 does not wait
  CHECK(plan_row_launch(f).traced);
  CHECK(RT_TRACED_MIN_LAUNCHES == 8);
  // the decision reads nothing but the facts
  f = base(1);
  CHECK(plan_row_launch(f).traced == plan_row_launch(f).traced);
  printf("%d failures\n", fails);
  return fails != 0;
}
"""


def test_plan_truth_table_for_traced(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    (tmp_path / "h.cpp").write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", str(tmp_path / "h.cpp"), "-o",
                        str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]


def _program(text, t=0.0):
    import tinyraytracerinrust_amd as T
    s = T.Scene.compile(text, t, 64, 48, asset_dir=SCENES)
    assert s.status == 0, s.error
    return s.spec_program()


def _holds_pass(prog):
    """The program's one check kernel takes `mode` (and what an empty prim word gets) and hands both on."""
    n = prog.count("void rt_spec_lean_check(")
    assert n <= 1
    if not n:
        assert "int mode" not in prog
        return False
    k = prog[prog.index("void rt_spec_lean_check("):]
    k = k[:k.index("\n}\n")]
    assert "RtTileRec* __restrict__ recs, int mode, uint32_t keep_bit)" in k, k
    assert re.search(r"lean_check_body<(true|false)>\(S, y_first, band_rows, band_pitch, n_rows, recs, mode, keep_bit\);", k), k
    assert prog.count("int mode") == 1                           # no second kernel beside it
    return True


def test_program_text_holds_one_check_kernel_with_mode_where_lean_ok():
    import tinyraytracerinrust_amd as T
    prog = _program(scene_text("globes"))
    assert "constexpr bool LEAN_OK = true;" in prog and _holds_pass(prog)
    scene = FLOOR + "draw(sphere(<45, -8, 10>, 12, red, 0.3))\n"
    assert _holds_pass(_program(scene + LIGHT * 3))                                          # four lights
    for text, t in ((scene + LIGHT * 4, 0.0),                                                # a fifth light
                    ("draw(sphere(<0, 0, 0>, 30, red))", 0.0),                               # no mask plane
                    (scene_text("spinning_globes"), 0.3),                                    # refraction chains
                    (FLOOR + "draw(plane(<0, 0, -1>, 120, rgb(0.3, 0.5, 0.3), 0.2))\n" + scene + LIGHT, 0.0)):   # two planes
        prog = _program(text, t)
        assert "constexpr bool LEAN_OK = false;" in prog and not _holds_pass(prog)
    text = scene_text("spinning_globes")
    frames = [T.Scene.compile(text, f / 6, 64, 48, asset_dir=SCENES) for f in range(6)]
    T.Scene.clear_families()
    try:
        T.Scene.register_family(frames)
        prog = frames[2].spec_program()
        assert "#define RT_SPEC_FAMILY 1" in prog and not _holds_pass(prog)                  # a family program
    finally:
        T.Scene.clear_families()
    # the pass is one function behind the check's wave-uniform mode test, in the device code of the masked programs
    body = (CSRC / "rt_bodies.h").read_text()
    assert re.search(r"if \(__builtin_amdgcn_readfirstlane\(mode\) != 0\) \{\s+trace_masks_body<FC>\(", body)


def test_option_and_setter_are_declared():
    import tinyraytracerinrust_amd as T
    from tinyraytracerinrust_amd import _lib
    assert _lib.RT_OPT_TRACED_MASKS == 13
    abi = (ROOT / "include" / "rt_abi.h").read_text()
    assert re.search(r"RT_OPT_TRACED_MASKS = 13\b", abi)
    assert "int rt_ctx_tile_records(rt_ctx* ctx, uint32_t* words, size_t cap_entries, uint32_t* n_entries);" in abi
    assert callable(T.Renderer.set_traced_masks) and callable(T.Renderer.tile_records)
    assert hasattr(T.lib(), "rt_ctx_tile_records")
    assert "rt_ctx_tile_records" in _lib.SIGNATURES
