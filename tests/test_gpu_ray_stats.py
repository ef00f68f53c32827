"""Ray counts on the GPU (rt_count_rays, rt_count_rays_row_bands) against the CPU oracle: per pixel, per row and
per frame, every check an exact integer equality.

The per-pixel reference is the oracle's ray debugger: ``OracleScene.record_rays(x, y)`` viewed with the product's
RAY_RECORD_DTYPE gives primary / reflect / refract = the records of ray_type 0 / 1 / 2 and shadow = n_lights x the
records with ``intersected != 0`` (every light for every shaded hit, raytracer.rs:175).  Each reference's frame sums
are asserted equal to the counting oracle's ray_primary / ray_shadow / ray_reflect / ray_refract, so the reference
is itself checked on every run.

Shapes: 72x53 (partial 8x8 tiles in both directions) and 40x24 for the 170-object fractal; 41x21 for the two-eye
scenes (odd width: the stereoscopic seam at x = 20 and the odd last column).  A reference is computed once per
case, shared and read-only; the largest oracle loop is 3 816 record_rays calls."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, SCENES, scene_text
from tests.stereo_refs import EYE_DISTANCE, eye_centres, eye_oracle

pytestmark = pytest.mark.gpu

W, H = 72, 53
NAMES = ("primary", "shadow", "reflect", "refract")
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -6
LAYOUTS = [("cyclic", 3, 5), ("cyclic", 2, 8), ("contiguous", 3, 0)]        # tests/test_gpu_antialias_bands.py's
ROW_SENTINEL, PIXEL_SENTINEL = 0xA5A5A5A5A5A5A5A5, 0xDEADBEEF
# (scene, time, width, height, depth)
CASES = [("globes", 0.0, W, H, 10), ("globes", 0.0, W, H, 0), ("spinning_globes", 0.1, W, H, 10),
         ("spinning_globes", 0.1, W, H, 3), ("three_cubes", 0.0, W, H, 10), ("fractal", 0.0, 40, 24, 4)]
RECORD_CAP = 1 << 12            # far above any pixel's ray tree here (at most 14 rays); checked below


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


def oracle_pixel(sc, x, y):
    """(primary, shadow, reflect, refract) of the oracle's get_pixel(x, y), from its ray records."""
    from tinyraytracerinrust_amd.raytracer import RAY_RECORD_DTYPE
    raw, _ = sc.record_rays(float(x), float(y), cap=RECORD_CAP)
    rec = raw.view(RAY_RECORD_DTYPE)
    assert len(rec) < RECORD_CAP
    t = rec["ray_type"]
    return (int((t == 0).sum()), sc.n_lights * int((rec["intersected"] != 0).sum()), int((t == 1).sum()),
            int((t == 2).sum()))


@functools.lru_cache(maxsize=None)
def reference(name, time, w, h, depth):
    """(h, w, 4) uint32 counts per pixel of the perspective frame, read-only; its sums checked against the counting
    oracle's own counters."""
    from oracle import oracle as O
    text = scene_text(name)
    sc = O.OracleScene(text, time, w, h, max_depth=depth)
    ref = np.array([[oracle_pixel(sc, x, y) for x in range(w)] for y in range(h)], np.uint32)
    cnt = O.OracleScene(text, time, w, h, max_depth=depth, counting=True).render()[2]
    sums = ref.sum(axis=(0, 1), dtype=np.uint64)
    print(f"{name} t={time} {w}x{h} depth {depth}: reference sums {sums.tolist()}, most rays on a pixel "
          f"{int(ref[..., [0, 2, 3]].sum(axis=-1).max())}")
    assert sums.tolist() == [cnt["ray_primary"], cnt["ray_shadow"], cnt["ray_reflect"], cnt["ray_refract"]]
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def two_eye_reference(kind, name, time, w, h, depth):
    """The same for a two-eye scene, composed as tests/stereo_refs.py point_reference composes colours:
    stereoscopic x >= w // 2 is the left eye's pixel x - w // 2, any other the right eye's; anaglyph both eyes'."""
    text = scene_text(name)
    left, right = eye_centres(text, time, EYE_DISTANCE)
    ew = w // 2 if kind == "stereoscopic" else w
    Ls, Rs = eye_oracle(text, time, ew, h, left, depth), eye_oracle(text, time, ew, h, right, depth)
    ref = np.zeros((h, w, 4), np.uint32)
    for y in range(h):
        for x in range(w):
            if kind == "stereoscopic":
                ref[y, x] = oracle_pixel(Ls, x - ew, y) if x >= ew else oracle_pixel(Rs, x, y)
            else:
                ref[y, x] = np.add(oracle_pixel(Ls, x, y), oracle_pixel(Rs, x, y))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def tracer(name, time, w, h, kind="perspective"):
    import tinyraytracerinrust_amd as T
    rt = T.RayTracer(w, h)
    rt.load_scene(scene_text(name), time, asset_dir=SCENES, camera_kind=kind,
                  eye_distance=EYE_DISTANCE if kind != "perspective" else None)
    return rt


def totals_of(res):
    return [res[k] for k in NAMES]


def check_against(res, ref, label):
    rows = ref.sum(axis=1, dtype=np.uint64)
    sums = ref.sum(axis=(0, 1), dtype=np.uint64).tolist()
    bad = int((res["pixels"] != ref).any(axis=-1).sum())
    print(f"{label}: totals {totals_of(res)} (reference {sums}), pixels that differ {bad}, "
          f"rows that differ {int((res['rows'] != rows).any(axis=-1).sum())}")
    assert res["pixels"].dtype == np.uint32 and res["rows"].dtype == np.uint64
    assert np.array_equal(res["pixels"], ref)
    assert np.array_equal(res["rows"], rows)
    assert totals_of(res) == sums
    assert res["total"] == sum(sums)


# ---------------------------------------------------------------- 1. per pixel, per row, per frame
@pytest.mark.parametrize("name,time,w,h,depth", CASES)
def test_counts_equal_the_oracle(T, worldmap, name, time, w, h, depth):
    ref = reference(name, time, w, h, depth)
    res = tracer(name, time, w, h).renderer.count_rays(0, h, max_depth=depth, rows=True, pixels=True)
    check_against(res, ref, f"{name} t={time} {w}x{h} depth {depth}")
    assert res["primary"] == w * h
    if depth == 0:
        assert res["reflect"] == res["refract"] == 0


def test_raytracer_counts_the_frame_at_its_depth(T, worldmap):
    rt = tracer("globes", 0.0, W, H)
    assert rt.max_depth == 10
    res = rt.count_rays()
    assert totals_of(res) == reference("globes", 0.0, W, H, 10).sum(axis=(0, 1), dtype=np.uint64).tolist()
    assert "rows" not in res and "pixels" not in res


# ---------------------------------------------------------------- 2. row bands
@pytest.fixture(scope="module")
def whole(T, worldmap):
    res = tracer("globes", 0.0, W, H).renderer.count_rays(rows=True, pixels=True)
    res["rows"].setflags(write=False)
    res["pixels"].setflags(write=False)
    return res


@pytest.mark.parametrize("layout,world,band", LAYOUTS)
def test_bands_equal_the_whole_frame(T, whole, layout, world, band):
    from tinyraytracerinrust_amd import distributed as D
    r = tracer("globes", 0.0, W, H).renderer
    slot_rows = D.rows_per_rank(H, world, layout, band)
    sums, owned, past = np.zeros(4, np.uint64), [], 0
    for rank in range(world):
        y_first, band_rows, pitch, n_bands = D.band_params(H, world, rank, layout, band)
        rows = np.full((slot_rows, 4), ROW_SENTINEL, np.uint64)
        pixels = np.full((slot_rows, W, 4), PIXEL_SENTINEL, np.uint32)
        res = r.count_rays_row_bands(y_first, band_rows, pitch, n_bands, out_rows=rows, out_pixels=pixels)
        assert res["rows"] is rows and res["pixels"] is pixels
        for p in range(slot_rows):
            b, j = divmod(p, band_rows) if band_rows else (n_bands, 0)
            y = y_first + b * pitch + j
            if b < n_bands and y < H:
                owned.append(y)
                assert np.array_equal(rows[p], whole["rows"][y]), (rank, p, y)
                assert np.array_equal(pixels[p], whole["pixels"][y]), (rank, p, y)
            else:                                   # a row at or past H, or past the rank's bands: never written
                past += 1
                assert (rows[p] == ROW_SENTINEL).all() and (pixels[p] == PIXEL_SENTINEL).all(), (rank, p)
        sums += np.array(totals_of(res), np.uint64)
        assert totals_of(res) == rows[rows[:, 0] != ROW_SENTINEL].sum(axis=0, dtype=np.uint64).tolist()
    print(f"{layout} world={world} band={band}: rank totals sum to {sums.tolist()}, rows left untouched {past}")
    assert sorted(owned) == list(range(H))
    assert past > 0
    assert sums.tolist() == totals_of(whole)


# ---------------------------------------------------------------- 3. two-eye scenes
@pytest.mark.parametrize("kind", ["stereoscopic", "anaglyph"])
def test_two_eye_scenes(T, worldmap, kind):
    w, h = 41, 21
    ref = two_eye_reference(kind, "globes", 0.1, w, h, 10)
    res = tracer("globes", 0.1, w, h, kind).renderer.count_rays(rows=True, pixels=True)
    check_against(res, ref, f"globes t=0.1 {w}x{h} {kind}")
    assert res["primary"] == (2 if kind == "anaglyph" else 1) * w * h


# ---------------------------------------------------------------- 4. pointers and arguments
def test_device_and_host_outputs_agree(T, whole):
    import torch
    r = tracer("globes", 0.0, W, H).renderer
    rows = torch.zeros((H, 4), dtype=torch.int64, device="cuda")
    pixels = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda")
    res = r.count_rays(out_rows=rows, out_pixels=pixels)
    assert res["rows"] is rows and res["pixels"] is pixels
    assert totals_of(res) == totals_of(whole)
    assert np.array_equal(rows.cpu().numpy().view(np.uint64), whole["rows"])
    assert np.array_equal(pixels.cpu().numpy().view(np.uint32), whole["pixels"])
    # no totals: asynchronous on the stream; a padded device row stride; `rows` still holds the first call's sums,
    # which the library must clear before it adds
    padded = torch.full((H, W + 3, 4), -1, dtype=torch.int32, device="cuda")
    res = r.count_rays(out_rows=rows, out_pixels=padded[:, :W], totals=False)
    assert "primary" not in res
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint64), whole["rows"])
    assert np.array_equal(padded[:, :W].cpu().numpy().view(np.uint32), whole["pixels"])
    assert (padded[:, W:] == -1).all()


def test_each_output_alone(T, whole):
    r = tracer("globes", 0.0, W, H).renderer
    res = r.count_rays()
    assert totals_of(res) == totals_of(whole) and set(res) == set(NAMES) | {"total"}
    res = r.count_rays(rows=True, totals=False)
    assert set(res) == {"rows"} and np.array_equal(res["rows"], whole["rows"])
    res = r.count_rays(pixels=True, totals=False)
    assert set(res) == {"pixels"} and np.array_equal(res["pixels"], whole["pixels"])
    res = r.count_rays(10, 31, rows=True)               # a row range: its rows, its sums
    assert np.array_equal(res["rows"], whole["rows"][10:31])
    assert totals_of(res) == whole["rows"][10:31].sum(axis=0, dtype=np.uint64).tolist()


def test_argument_errors(T, whole):
    r = tracer("globes", 0.0, W, H).renderer
    lib, t = T.lib(), T._lib.rt_ray_counts()
    tp = ctypes.byref(t)
    assert lib.rt_count_rays(r.h, 0, H, -1, None, None, None, 0, None) == RT_ERR_INVALID          # all outputs NULL
    assert lib.rt_count_rays_row_bands(r.h, 0, 8, 8, 1, -1, None, None, None, 0, None) == RT_ERR_INVALID
    assert lib.rt_count_rays_row_bands(r.h, 0, 8, 4, 2, -1, tp, None, None, 0, None) == RT_ERR_INVALID   # pitch < rows
    assert lib.rt_count_rays_row_bands(r.h, H, 8, 8, 1, -1, tp, None, None, 0, None) == RT_ERR_INVALID   # y_first >= H
    assert lib.rt_count_rays_row_bands(r.h, 0, 8, 8, 1, 17, tp, None, None, 0, None) == RT_ERR_UNSUPPORTED
    assert lib.rt_count_rays(r.h, 0, H, 17, tp, None, None, 0, None) == RT_ERR_UNSUPPORTED
    assert lib.rt_count_rays(r.h, 5, H + 1, -1, tp, None, None, 0, None) == RT_ERR_INVALID
    px = np.zeros((8, W, 4), np.uint32)
    assert lib.rt_count_rays(r.h, 0, 8, -1, None, None, ctypes.c_void_p(px.ctypes.data), W * 16 - 4, None) == RT_ERR_INVALID
    fresh = T.Renderer(0)                                                                   # no uploaded scene
    assert lib.rt_count_rays(fresh.h, 0, 1, -1, tp, None, None, 0, None) == RT_ERR_INVALID
    fresh.free()
    for zero in ((0, 0, 8, 1), (0, 8, 8, 0)):                                               # no rows: zeros, RT_OK
        t.primary = t.shadow = t.reflect = t.refract = 77
        assert lib.rt_count_rays_row_bands(r.h, *zero, -1, tp, None, None, 0, None) == 0
        assert (t.primary, t.shadow, t.reflect, t.refract) == (0, 0, 0, 0)
    res = r.count_rays_row_bands(0, 8, 8, 0, rows=True, pixels=True)
    assert res["total"] == 0 and res["rows"].shape == (0, 4) and res["pixels"].shape == (0, W, 4)


# ---------------------------------------------------------------- 5. no side effects
def test_a_count_changes_no_later_render(T, worldmap):
    import tinyraytracerinrust_amd as Tm
    rt = Tm.RayTracer(W, H)                              # a renderer of its own: its launch history is this test's
    rt.load_scene(scene_text("globes"), 0.0, asset_dir=SCENES)
    r = rt.renderer
    before = r.render_rows_host(0, H)
    info = r.kernel_info()
    assert "last launch: " in info
    res = r.count_rays(rows=True, pixels=True)
    assert res["primary"] == W * H
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]
    assert r.last_kernel_ms() > 0.0                       # the count's own launch is timed
    after = r.render_rows_host(0, H)
    assert np.array_equal(before, after)
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]


# ---------------------------------------------------------------- 6. the headless driver
def test_cli_counts_and_ray_map(T, whole, tmp_path):
    out, ray_map = tmp_path / "globes.png", tmp_path / "rays.png"
    p = subprocess.run([sys.executable, "-m", "tinyraytracerinrust_amd", "render", os.path.join(SCENES, "globes.scene"),
                        "--size", f"{W}x{H}", "--count-rays", "--ray-map", str(ray_map), "-o", str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stderr.strip().splitlines()[-1])
    assert info["rays"] == dict(zip(NAMES, totals_of(whole)), total=whole["total"])
    assert info["rays_per_pixel"] == round(whole["total"] / (W * H), 3)
    assert info["count_ms"] > 0
    n = whole["pixels"].sum(axis=-1, dtype=np.uint64)
    want = (255 * n // n.max()).astype(np.uint8)          # floor(255 * n / max n), in integers
    got = T.read_png_rgba8(str(ray_map))
    assert got.shape == (H, W, 4)
    for ch in range(3):
        assert np.array_equal(got[..., ch], want)
    assert out.exists()
