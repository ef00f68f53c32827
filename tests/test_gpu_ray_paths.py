"""Ray paths for many samples in one launch (rt_ray_paths_offsets, rt_ray_paths; k_paths.hip) against the CPU oracle's
``record_rays`` per sample, against the one-sample recorder rt_record_rays, and against the GPU's own ray counts and
sample colours.

Shapes: a 72x53 frame (partial 8x8 tiles both ways).  The samples are its 3 816 pixel centres, row-major, plus 300
fractional positions from a seeded generator: 4 116 samples, no multiple of 64 or 256 and five scan blocks of 1 024.
The scenes: globes (reflection-only), spinning_globes at t 0.5 (refraction chains), fractal (ray trees, 171 objects),
three_cubes and two seeded fuzz scenes (a tree and a chain scene), so every wave carries mixed segment lengths.  One
oracle pass and one GPU call per scene, shared by the checks and read-only.

Checks: segment lengths and every geometric field are exact equalities; colours are within 1e-9 of the oracle's
(tests/test_gpu_antialias.py test_ray_debugger_records' tolerance) and bit for bit those of rt_record_rays and
rt_render_points_f64."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, SCENES, scene_text
from tests.scene_fuzz import random_scene

pytestmark = pytest.mark.gpu

W, H = 72, 53
RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, -1, -6
FIELDS = ("depth", "ray_type", "object", "intersected", "has_normal", "point", "direction", "distance", "intersection",
          "normal")
# (name, time): the fuzz scenes by seed -- tests/test_gpu_side_fuzz.py's stand-ins with 8 and 7 rays on a pixel
CASES = [("globes", 0.0), ("spinning_globes", 0.5), ("fractal", 0.0), ("three_cubes", 0.0), ("fuzz_tree_6028", 0.0),
         ("fuzz_chain_6118", 0.0)]
IDS = [c[0] for c in CASES]
PATTERN = 0xA5


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


def text_of(name):
    if name.startswith("fuzz_tree_"):
        return random_scene(int(name.rsplit("_", 1)[1]))
    if name.startswith("fuzz_chain_"):
        return random_scene(int(name.rsplit("_", 1)[1]), chains=True)
    return scene_text(name)


@functools.lru_cache(maxsize=None)
def samples():
    """The frame's pixel centres, row-major, then 300 fractional positions inside it: (4116, 2) f64."""
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([xs.ravel(), ys.ravel()], axis=-1).astype(np.float64)
    frac = np.random.default_rng(20261021).uniform([0.0, 0.0], [W - 1.0, H - 1.0], size=(300, 2))
    xy = np.ascontiguousarray(np.concatenate([centres, frac]))
    assert xy.shape == (4116, 2) and xy.shape[0] % 64 and xy.shape[0] > 4 * 1024
    xy.setflags(write=False)
    return xy


@functools.lru_cache(maxsize=None)
def reference(name, time, max_depth=10):
    """The oracle's records of every sample: offsets (n + 1), the records back to back, the colours."""
    from oracle import oracle as O
    from tinyraytracerinrust_amd.raytracer import RAY_RECORD_DTYPE
    O.register_texture_file("worldmap.png", os.path.join(SCENES, "worldmap.png"))
    sc = O.OracleScene(text_of(name), time, W, H, max_depth=max_depth)
    xy = samples()
    recs, rgba = [], np.zeros((len(xy), 4))
    for i, (x, y) in enumerate(xy):
        raw, rgba[i] = sc.record_rays(float(x), float(y), cap=1 << 12)
        recs.append(np.frombuffer(raw.tobytes(), RAY_RECORD_DTYPE))
    counts = np.array([len(r) for r in recs], np.uint64)
    assert counts.min() >= 1 and counts.max() < (1 << 12)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ref = {"offsets": offsets, "records": np.concatenate(recs), "rgba": rgba}
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def tracer(name, time, camera="perspective"):
    import tinyraytracerinrust_amd as T
    rt = T.RayTracer(W, H)
    rt.load_scene(text_of(name), time, asset_dir=SCENES, camera_kind=camera, eye_distance=None if camera == "perspective" else 4.0)
    return rt


@functools.lru_cache(maxsize=None)
def gpu(name, time):
    """Renderer.ray_paths over every sample, once per scene."""
    res = tracer(name, time).renderer.ray_paths(samples())
    for a in res.values():
        a.setflags(write=False)
    return res


def segment(res, i):
    return res["records"][int(res["offsets"][i]):int(res["offsets"][i + 1])]


# ---------------------------------------------------------------- 0. the references are what the issue measured
def test_the_references_are_not_vacuous():
    n_px = W * H
    want = {"globes": (6072, 1, 6, None), "spinning_globes": (10776, 1, 11, None), "fractal": (10360, 1, 34, 27),
            "three_cubes": (7475, None, None, None)}
    for name, time in CASES:
        counts = np.diff(reference(name, time)["offsets"])[:n_px]
        print(f"{name}: {int(counts.sum())} records at the pixel centres, {int(counts.min())}-{int(counts.max())} per "
              f"sample, {np.unique(counts).size} distinct counts")
        if name in want:
            total, lo, hi, distinct = want[name]
            assert int(counts.sum()) == total
            assert lo is None or (int(counts.min()), int(counts.max())) == (lo, hi)
            assert distinct is None or np.unique(counts).size == distinct
        else:
            assert counts.max() >= 3                                   # the fuzz scenes branch too
        blocks = counts[:n_px - n_px % 64].reshape(-1, 64)
        assert (blocks.min(axis=1) != blocks.max(axis=1)).any()        # waves with mixed segment lengths


# ---------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("name,time", CASES, ids=IDS)
def test_records_equal_the_oracle(T, name, time):
    ref, got = reference(name, time), gpu(name, time)
    assert got["offsets"].dtype == np.uint64 and got["records"].dtype == T.RAY_RECORD_DTYPE
    assert np.array_equal(got["offsets"], ref["offsets"])             # every segment length
    assert len(got["records"]) == int(ref["offsets"][-1]) == len(ref["records"])
    for f in FIELDS:
        assert np.array_equal(got["records"][f], ref["records"][f]), f
    dc = np.abs(got["records"]["color"] - ref["records"]["color"]).max()
    dp = np.abs(got["rgba"] - ref["rgba"]).max()
    print(f"{name}: max |colour - oracle| {dc:.3e}, max |rgba - oracle| {dp:.3e}")
    assert dc <= 1e-9 and dp <= 1e-9
    last = got["records"]["color"][got["offsets"][1:].astype(np.int64) - 1]   # the primary ray reports last
    assert np.array_equal(got["rgba"], last)
    assert (got["records"]["depth"][got["offsets"][1:].astype(np.int64) - 1] == 0).all()
    assert (got["records"]["pad"] == 0).all()


# ---------------------------------------------------------------- 2. the one-sample recorder
@pytest.mark.parametrize("name,time", CASES, ids=IDS)
def test_records_equal_rt_record_rays_bit_for_bit(T, name, time):
    got, xy = gpu(name, time), samples()
    counts = np.diff(got["offsets"]).astype(np.int64)
    picks = set(np.random.default_rng(7).choice(len(xy), 34, replace=False).tolist())
    picks |= {int(np.argmax(counts)), len(xy) - 1}                    # the longest path, the last (fractional) sample
    r = tracer(name, time).renderer
    for i in sorted(picks):
        one, rgba = r.record_rays(float(xy[i, 0]), float(xy[i, 1]), cap=1 << 12)
        seg = segment(got, i)
        assert len(one) == len(seg), i
        for f in FIELDS + ("color",):
            assert one[f].tobytes() == seg[f].tobytes(), (i, f)
        assert rgba.tobytes() == got["rgba"][i].tobytes(), i


# ---------------------------------------------------------------- 3. cross-checks on the GPU
@pytest.mark.parametrize("name,time", CASES, ids=IDS)
def test_counts_and_colours_equal_the_other_entries(T, name, time):
    got = gpu(name, time)
    r = tracer(name, time).renderer
    px = r.count_rays(pixels=True)["pixels"].astype(np.uint64)        # (H, W, 4): primary, shadow, reflect, refract
    rays = (px[..., 0] + px[..., 2] + px[..., 3]).ravel()
    assert np.array_equal(np.diff(got["offsets"])[:W * H], rays)
    assert np.array_equal(r.ray_paths_offsets(samples()), got["offsets"])
    assert r.render_points(samples()).tobytes() == got["rgba"].tobytes()


# ---------------------------------------------------------------- 4. shapes and pointers
def raw_calls(T, r, xy, where, max_depth=-1, stream=None):
    """Both calls with every buffer on the host ("host"), on the device ("device": torch buffers, the first call
    asynchronous, total NULL) or mixed ("mix": xy and records on the device, offsets and colours on the host).
    Returns (status of the second call, offsets, records as bytes, rgba) as numpy arrays."""
    import torch
    lib, n = T.lib(), len(xy)
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else 0)
    on_dev = {"host": set(), "device": {"xy", "offsets", "records", "rgba"}, "mix": {"xy", "records"}}[where]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with ctx:
        xy_t = torch.from_numpy(np.array(xy, np.float64).reshape(-1, 2))
        off_t = torch.full((n + 1,), -1, dtype=torch.int64)
        rgba_t = torch.full((max(n, 1), 4), -2.5, dtype=torch.float64)
        if "xy" in on_dev:
            xy_t = xy_t.to(dev)
        if "offsets" in on_dev:
            off_t = off_t.to(dev)
        if "rgba" in on_dev:
            rgba_t = rgba_t.to(dev)
        total = ctypes.c_uint64(0xDEAD)
        use_total = "offsets" not in on_dev
        if stream is None:
            torch.cuda.synchronize()
        rc = lib.rt_ray_paths_offsets(r.h, ctypes.c_void_p(xy_t.data_ptr()), n, max_depth, ctypes.c_void_p(off_t.data_ptr()),
                                      ctypes.byref(total) if use_total else None, st)
        assert rc == RT_OK, lib.rt_last_error()
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        m = int(off_t[n].item())
        if use_total:
            assert total.value == m
        rec_t = torch.full((max(m, 1) * 160,), PATTERN, dtype=torch.uint8)
        if "records" in on_dev:
            rec_t = rec_t.to(dev)
            torch.cuda.synchronize()
        rc = lib.rt_ray_paths(r.h, ctypes.c_void_p(xy_t.data_ptr()), n, max_depth, ctypes.c_void_p(off_t.data_ptr()),
                              ctypes.c_void_p(rec_t.data_ptr()), m, ctypes.c_void_p(rgba_t.data_ptr()), st)
        torch.cuda.synchronize()
    return rc, off_t.cpu().numpy().astype(np.uint64), rec_t.cpu().numpy()[:m * 160], rgba_t.cpu().numpy()[:n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes_and_pointers(T, n):
    """n around a wave and a workgroup, three ways: equal byte for byte, and equal to the big call's segments."""
    import torch
    name, time = "fractal", 0.0
    big, r = gpu(name, time), tracer(name, time).renderer
    first = 1700                                                       # a stretch of the frame with ray trees in it
    xy = samples()[first:first + n]
    runs = {w: raw_calls(T, r, xy, w) for w in ("host", "device", "mix")}
    runs["stream"] = raw_calls(T, r, xy, "device", stream=torch.cuda.Stream())
    for w, (rc, offsets, records, rgba) in runs.items():
        assert rc == RT_OK, w
        assert offsets[0] == 0 and len(records) == int(offsets[n]) * 160
        for k, a in enumerate((offsets, records, rgba)):
            assert a.tobytes() == runs["host"][k + 1].tobytes(), (w, k)
    _, offsets, records, rgba = runs["host"]
    base = int(big["offsets"][first])
    assert np.array_equal(offsets, big["offsets"][first:first + n + 1] - np.uint64(base))
    want = big["records"][base:base + int(offsets[n])]
    assert records.tobytes() == want.tobytes()
    assert rgba.tobytes() == big["rgba"][first:first + n].tobytes()
    if n:
        assert np.unique(np.diff(offsets)).size >= (1 if n == 1 else 2)     # mixed lengths in the stretch
    assert r.ray_paths(xy)["records"].tobytes() == want.tobytes()          # the wrapper, n == 0 included


def test_no_samples_write_nothing(T):
    lib, r = T.lib(), tracer("globes", 0.0).renderer
    offsets = np.full(1, 77, np.uint64)
    total = ctypes.c_uint64(77)
    assert lib.rt_ray_paths_offsets(r.h, None, 0, -1, ctypes.c_void_p(offsets.ctypes.data), ctypes.byref(total), None) == RT_OK
    assert offsets[0] == 0 and total.value == 0
    records = np.full(160, PATTERN, np.uint8)
    rgba = np.full(4, -2.5)
    assert lib.rt_ray_paths(r.h, None, 0, -1, ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(records.ctypes.data), 1,
                            ctypes.c_void_p(rgba.ctypes.data), None) == RT_OK
    assert (records == PATTERN).all() and (rgba == -2.5).all()
    res = r.ray_paths(np.zeros((0, 2)))
    assert res["offsets"].tolist() == [0] and res["records"].shape == (0,) and res["rgba"].shape == (0, 4)


# ---------------------------------------------------------------- 5. depths
def test_depth_zero_is_one_record_per_sample(T):
    r = tracer("fractal", 0.0).renderer
    res = r.ray_paths(samples(), max_depth=0)
    assert np.array_equal(res["offsets"], np.arange(len(samples()) + 1, dtype=np.uint64))
    assert (res["records"]["depth"] == 0).all() and (res["records"]["ray_type"] == 0).all()
    assert np.array_equal(res["rgba"], res["records"]["color"])


def test_depth_two_equals_the_oracle_at_that_depth(T):
    ref = reference("fractal", 0.0, 2)
    got = tracer("fractal", 0.0).renderer.ray_paths(samples(), max_depth=2)
    assert np.array_equal(got["offsets"], ref["offsets"])
    assert ref["offsets"][-1] < reference("fractal", 0.0)["offsets"][-1]       # the depth cuts trees
    assert got["records"]["depth"].max() == 2
    for f in FIELDS:
        assert np.array_equal(got["records"][f], ref["records"][f]), f
    assert np.abs(got["records"]["color"] - ref["records"]["color"]).max() <= 1e-9
    assert np.abs(got["rgba"] - ref["rgba"]).max() <= 1e-9


# ---------------------------------------------------------------- 6. stale offsets
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", ["another_depth", "short_cap"])
def test_stale_offsets_are_refused_and_clamped(T, case, where):
    """Offsets that do not fit the call: RT_ERR_INVALID, nothing written past cap_records, and every sample whose
    segment was exact holds the clean run's records.  The buffer (total + 64 records) would hold a correct run."""
    import torch
    lib = T.lib()
    name, time = "fractal", 0.0
    clean, r, xy = gpu(name, time), tracer(name, time).renderer, samples()
    n, total = len(xy), int(clean["offsets"][-1])
    counts = np.diff(clean["offsets"]).astype(np.int64)
    if case == "another_depth":
        offsets = r.ray_paths_offsets(xy, max_depth=2)
        cap = int(offsets[-1])
        assert cap < total
    else:
        offsets = clean["offsets"].copy()
        cap = total - 5
    seg_end = np.minimum(offsets[1:], np.uint64(cap)).astype(np.int64)
    seg_len = np.maximum(seg_end - offsets[:-1].astype(np.int64), 0)
    exact = seg_len == counts
    assert exact.any() and not exact.all()
    buf = torch.full(((total + 64) * 160,), PATTERN, dtype=torch.uint8)
    if where == "device":
        buf = buf.to(torch.device("cuda", 0))
        torch.cuda.synchronize()
    rgba = np.zeros((n, 4))
    rc = lib.rt_ray_paths(r.h, ctypes.c_void_p(xy.ctypes.data), n, -1, ctypes.c_void_p(offsets.ctypes.data),
                          ctypes.c_void_p(buf.data_ptr()), cap, ctypes.c_void_p(rgba.ctypes.data), None)
    assert rc == RT_ERR_INVALID
    assert b"offsets" in lib.rt_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[cap * 160:] == PATTERN).all()                          # nothing past cap_records
    recs = out[:cap * 160].view(T.RAY_RECORD_DTYPE)
    for i in np.flatnonzero(exact):
        a, b = int(offsets[i]), int(clean["offsets"][i])
        assert recs[a:a + counts[i]].tobytes() == clean["records"][b:b + counts[i]].tobytes(), i
    assert rgba.tobytes() == clean["rgba"].tobytes()                   # the colours do not depend on the segments
    # the context is as good as before: the clean call again
    again = r.ray_paths(xy[:300])
    assert again["records"].tobytes() == clean["records"][:int(clean["offsets"][300])].tobytes()


# ---------------------------------------------------------------- 7. the other contract cases
def test_argument_errors(T):
    lib = T.lib()
    xy = np.array([[3.0, 4.0], [5.5, 6.25]])
    offsets = np.full(3, 77, np.uint64)
    records = np.full(64 * 160, PATTERN, np.uint8)
    total = ctypes.c_uint64(77)
    xp, op, rp = (ctypes.c_void_p(a.ctypes.data) for a in (xy, offsets, records))

    def both(h, n=2, depth=-1):
        return (lib.rt_ray_paths_offsets(h, xp, n, depth, op, ctypes.byref(total), None),
                lib.rt_ray_paths(h, xp, n, depth, op, rp, 64, None, None))
    r = tracer("globes", 0.0).renderer
    assert both(r.h, depth=17) == (RT_ERR_UNSUPPORTED, RT_ERR_UNSUPPORTED)                 # above RT_MAX_DEPTH_CAP
    for camera in ("stereoscopic", "anaglyph"):
        two = tracer("globes", 0.0, camera).renderer
        assert both(two.h) == (RT_ERR_UNSUPPORTED, RT_ERR_UNSUPPORTED)
        assert b"two-eye" in lib.rt_last_error()
        with pytest.raises(T.RtError) as e:
            two.ray_paths(xy)
        assert e.value.status == RT_ERR_UNSUPPORTED
    fresh = T.Renderer(0)                                                                  # no scene uploaded
    assert both(fresh.h) == (RT_ERR_INVALID, RT_ERR_INVALID)
    assert both(fresh.h, n=0) == (RT_ERR_INVALID, RT_ERR_INVALID)
    fresh.free()
    assert both(None) == (RT_ERR_INVALID, RT_ERR_INVALID)
    assert lib.rt_ray_paths_offsets(r.h, None, 2, -1, op, None, None) == RT_ERR_INVALID
    assert lib.rt_ray_paths_offsets(r.h, xp, 2, -1, None, ctypes.byref(total), None) == RT_ERR_INVALID
    assert lib.rt_ray_paths(r.h, xp, 2, -1, None, rp, 64, None, None) == RT_ERR_INVALID
    assert lib.rt_ray_paths(r.h, xp, 2, -1, op, None, 64, None, None) == RT_ERR_INVALID
    assert lib.rt_ray_paths_offsets(r.h, xp, (1 << 26) + 1, -1, op, None, None) == RT_ERR_UNSUPPORTED   # the scan's bound
    assert (offsets == 77).all() and total.value == 77 and (records == PATTERN).all()


def test_ray_paths_change_no_later_render(T):
    import tinyraytracerinrust_amd as Tm
    rt = Tm.RayTracer(W, H)                              # a renderer of its own: its launch history is this test's
    rt.load_scene(scene_text("globes"), 0.0, asset_dir=SCENES)
    r = rt.renderer
    before = r.render_rows_host(0, H)
    info = r.kernel_info()
    assert "last launch: " in info
    offsets = r.ray_paths_offsets(samples())
    assert r.last_kernel_ms() > 0.0                       # each call's own launches are timed
    assert np.array_equal(offsets, gpu("globes", 0.0)["offsets"])
    res = rt.ray_paths(samples())
    assert r.last_kernel_ms() > 0.0
    assert res["records"].tobytes() == gpu("globes", 0.0)["records"].tobytes()
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]
    after = r.render_rows_host(0, H)
    assert np.array_equal(before, after)
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]
    dbg = Tm.RayDebugger(W, H)                            # the debugger's many-sample form
    off = dbg.record_rays_many(rt, samples()[:200])
    assert np.array_equal(off, res["offsets"][:201])
    assert dbg.rays.tobytes() == res["records"][:int(off[-1])].tobytes()


# ---------------------------------------------------------------- 8. the headless driver
def test_cli_writes_the_paths(T, tmp_path):
    out, npz = tmp_path / "globes.png", tmp_path / "paths.npz"
    cmd = [sys.executable, "-m", "tinyraytracerinrust_amd", "render", os.path.join(SCENES, "globes.scene"),
           "--size", f"{W}x{H}", "-o", str(out), "--ray-paths", str(npz), "--ray-paths-step", "5"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stderr.strip().splitlines()[-1])
    got = np.load(npz)
    xy = np.array([[x, y] for y in range(0, H, 5) for x in range(0, W, 5)], np.float64)
    assert np.array_equal(got["xy"], xy)
    want = tracer("globes", 0.0).renderer.ray_paths(xy)
    assert np.array_equal(got["offsets"], want["offsets"])
    assert got["records"].dtype == T.RAY_RECORD_DTYPE and got["records"].tobytes() == want["records"].tobytes()
    assert info["ray_paths"]["points"] == len(xy) and info["ray_paths"]["records"] == len(want["records"])
    assert info["ray_paths"]["ms"] > 0
    assert out.exists()
