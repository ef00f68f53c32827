"""Lean tiles (RT_OPT_LEAN_TILES) on the CPU: which programs hold the lean kernel and the megakernel's lean
exit (spec_text.cpp), when a launch takes them (launch_plan.h plan_row_launch), and the option's declarations.
The pixels are checked on the GPU (tests/test_gpu_lean_tiles.py)."""
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


def _program(text, t=0.0):
    import tinyraytracerinrust_amd as T
    s = T.Scene.compile(text, t, 64, 48, asset_dir=SCENES)
    assert s.status == 0, s.error
    return s.spec_program()


def _holds_lean(prog):
    kernel = "void rt_spec_lean_0(" in prog and "void rt_spec_lean_check(" in prog
    exit_ = "constexpr bool LEAN_OK = true;" in prog
    assert kernel == exit_, "the lean kernel and the megakernel's exit go together"
    assert ("void rt_spec_lean_1(" in prog) == kernel             # the program text is level 2: the f64 form too
    assert "constexpr bool LEAN_OK = " in prog                    # every prelude says which
    return kernel


def test_program_text_holds_the_lean_kernel_where_the_class_exists():
    prog = _program(scene_text("globes"))
    assert _holds_lean(prog)
    k = prog[prog.index("void rt_spec_lean_0("):]
    k = k[:k.index("\n}\n")]
    assert "amdgpu_waves_per_eu(8)" in prog[prog.index("void rt_spec_lean_0(") - 120:prog.index("void rt_spec_lean_0(")]
    assert "lean_body<false, " in k and "RT_REC_PARAMS" in k and "RT_REC_ARGS" in k and "max_depth" in k   # the records, the runtime depth
    assert "rt_spec_lean_00" not in prog and "rt_spec_lean_01" not in prog   # no calibrating form
    # the exit sits in the device code under the same condition, not in the calibrating or primary-ray kernels
    body = (CSRC / "rt_bodies.h").read_text()
    assert re.search(r"if constexpr \(rt_spec::LEAN_OK && !CAL && !PRIM && MODE == RT_MODE_REFL\)\s+if \(R->x0 < 0\) return;", body)
    # a floor with boxed objects and up to four lights (the scene's own and three appended) holds it; a fifth
    # light does not (four shadow words)
    scene = FLOOR + "draw(sphere(<45, -8, 10>, 12, red, 0.3))\n"
    four, five = _program(scene + LIGHT * 3), _program(scene + LIGHT * 4)
    assert "N_LIGHTS = 4," in four and _holds_lean(four)
    assert "N_LIGHTS = 5," in five and not _holds_lean(five)


def test_program_text_holds_none_elsewhere():
    import tinyraytracerinrust_amd as T
    assert not _holds_lean(_program("draw(sphere(<0, 0, 0>, 30, red))"))                     # no mask plane
    assert not _holds_lean(_program(scene_text("spinning_globes"), 0.3))                     # refraction chains
    two_planes = FLOOR + "draw(plane(<0, 0, -1>, 120, rgb(0.3, 0.5, 0.3), 0.2))\ndraw(sphere(<45, -8, 10>, 12, red, 0.3))\n" + LIGHT
    assert not _holds_lean(_program(two_planes))                                             # a second unbounded object
    text = scene_text("spinning_globes")
    frames = [T.Scene.compile(text, f / 6, 64, 48, asset_dir=SCENES) for f in range(6)]
    T.Scene.clear_families()
    try:
        T.Scene.register_family(frames)
        prog = frames[2].spec_program()
        assert "#define RT_SPEC_FAMILY 1" in prog and not _holds_lean(prog)                  # a family program
    finally:
        T.Scene.clear_families()


HARNESS = r"""
#include "launch_plan.h"
#include <cstdio>
using namespace rt;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)
// globes-like: reflection-only, the single-scene program loaded with every kind, masks forced, the megakernel pinned
static LaunchFacts base() {
  LaunchFacts f = {};
  f.colour_fast = true; f.n_lights = 2; f.n_objects = 6;
  f.kernel_opt = RT_KERNEL_MEGA; f.tile_order = true; f.tile_masks = 2; f.tile_records = f.sky_fill = f.fast_clamp = true;
  f.sky_ok = f.masks_ok = true;
  f.max_depth = 5; f.n_tiles = 30000; f.slot = LaunchFacts::ORDERED; f.masks_pay = true;
  f.sh_trcap = 128; f.split_tile_mask = 0xFFFFFu; f.pool_byte_index = true;
  f.loaded = true; f.mode = RT_MODE_REFL; f.fc = true;
  for (int k = 0; k < SPEC_KINDS; ++k) f.has[k] = true;
  f.has_rows_ordered = true;
  f.lean_tiles = f.has_lean = true;
  return f;
}
int main() {
  LaunchFacts z = {};
  CHECK(!z.lean_tiles && !z.has_lean);                             // new members default to false
  LaunchPlan pz = {};
  CHECK(!pz.lean);
  LaunchFacts f = base();
  LaunchPlan p = plan_row_launch(f);
  CHECK(p.lean && p.records && p.masks && p.kind == SPEC_ROWS && p.path == LaunchPlan::MEGA);
  f = base(); f.slot = LaunchFacts::NONE;                          // an unordered launch reads records too
  CHECK(plan_row_launch(f).lean);
  f = base(); f.slot = LaunchFacts::CALIBRATING;                   // calibrating: cost[tile] is a tile's full time
  p = plan_row_launch(f);
  CHECK(!p.lean && p.records);
  f = base(); f.tile_records = false;                              // without records
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.tile_masks = 0;                                    // the mask-free megakernel
  p = plan_row_launch(f);
  CHECK(!p.lean && p.kind == SPEC_ROWS_NOMASK);
  f = base(); f.lean_tiles = false;                                // the option
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.has_lean = false;                                  // the program holds no lean kernel
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.max_depth = 0;                                     // the primary-ray path
  p = plan_row_launch(f);
  CHECK(!p.lean && p.path == LaunchPlan::PRIMARY && p.records);
  f = base(); f.kernel_opt = RT_KERNEL_DEFERRED;                   // the deferred path
  p = plan_row_launch(f);
  CHECK(!p.lean && p.path == LaunchPlan::DEFERRED);
  f = base(); f.kernel_opt = RT_KERNEL_AUTO; f.slot_deferred = true;
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.kernel_opt = RT_KERNEL_WAVEFRONT;
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.loaded = false;                                    // the generic kernels
  CHECK(!plan_row_launch(f).lean);
  f = base(); f.family = true;
  CHECK(!plan_row_launch(f).lean);
  printf("%d failures\n", fails);
  return fails != 0;
}
"""


def test_plan_takes_lean_only_on_the_masked_megakernel_with_records(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    (tmp_path / "h.cpp").write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", str(tmp_path / "h.cpp"), "-o",
                        str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(tmp_path / "h")], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]


def test_option_and_setter_are_declared():
    import tinyraytracerinrust_amd as T
    from tinyraytracerinrust_amd import _lib
    assert _lib.RT_OPT_LEAN_TILES == 12
    abi = (ROOT / "include" / "rt_abi.h").read_text()
    assert re.search(r"RT_OPT_LEAN_TILES = 12\b", abi)
    assert "int rt_scene_lean_report(const rt_scene* scene, char* buf, size_t cap, size_t* len);" in abi
    assert callable(T.Renderer.set_lean_tiles) and callable(T.Scene.lean_report)
    assert hasattr(T.lib(), "rt_scene_lean_report")
