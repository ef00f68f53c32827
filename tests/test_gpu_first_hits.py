"""First-hit maps on the GPU (rt_first_hits, rt_first_hits_row_bands, rt_first_hits_points) against the CPU oracle:
object, distance, occluded-light bits and raw normal of every pixel, every check an exact equality (integers equal,
doubles compared by their bytes).

The reference holds, per pixel, two oracle paths: ``orc_hit_signature(x, y)`` -- object, light mask and distance
(the reference's own nearest-hit and shadow loops, raytracer.rs:138-197) -- and the single record of
``OracleScene(..., max_depth=0).record_rays(x, y)`` -- object, distance and the shape's raw get_normal
(ray_debugger.rs:113-119).  Every reference asserts that the two paths agree on the object and on the distance's
bytes, so the reference is itself checked on every run, and each case asserts its own non-vacuity from the
reference alone.

Shapes: 72x53 (partial 8x8 tiles in both directions) and 40x24 for the 171-object fractal; 41x21 for the
stereoscopic scene (odd width: the seam at x = 20 and the odd last column).  A reference is computed once per
case, shared and read-only; the largest oracle loop is 3 816 pixels."""
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
PLANES = ("object", "distance", "shadow", "normal")
RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, -1, -6
LAYOUTS = [("cyclic", 3, 5), ("cyclic", 2, 8), ("contiguous", 3, 0)]        # tests/test_gpu_ray_stats.py's
# (scene, time, width, height, objects, lights, has a miss)
CASES = [("globes", 0.0, W, H, 6, 2, True), ("spinning_globes", 0.1, W, H, 4, 1, True),
         ("three_cubes", 0.0, W, H, 4, 2, True), ("fractal", 0.0, 40, 24, 171, 2, True),
         ("spinning_gimbals", 0.2, W, H, 10, 2, False)]
DTYPES = {"object": np.int32, "distance": np.float64, "shadow": np.uint32, "normal": np.float64}
SENTINELS = {"object": -7, "distance": -1.5, "shadow": 0xDEADBEEF, "normal": -2.5}


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


def oracle_sample(sc, x, y):
    """(object, distance, occluded-light mask, raw normal) of the oracle's get_pixel(x, y), from hit_signature and the
    depth-0 ray record; the two paths must agree on the object and on the distance's bytes."""
    from tinyraytracerinrust_amd.raytracer import RAY_RECORD_DTYPE
    t = ctypes.c_double(0.0)
    sig = int(sc.lib.orc_hit_signature(sc.h, float(x), float(y), ctypes.byref(t)))
    obj, mask = (-1, 0) if sig < 0 else ((sig % 4096) - 1, sig // 4096)
    raw, _ = sc.record_rays(float(x), float(y), cap=4)
    rec = raw.view(RAY_RECORD_DTYPE)
    assert len(rec) == 1 and rec["depth"][0] == 0 and rec["ray_type"][0] == 0
    assert int(rec["object"][0]) == obj, (x, y, obj, int(rec["object"][0]))
    assert np.float64(t.value).tobytes() == rec["distance"][0].tobytes(), (x, y, t.value, rec["distance"][0])
    assert bool(rec["has_normal"][0]) == (obj >= 0)
    return obj, t.value, mask, rec["normal"][0].copy()


def sample_planes(samples):
    """A list of oracle_sample results as the four planes (flat)."""
    ref = {"object": np.array([s[0] for s in samples], np.int32),
           "distance": np.array([s[1] for s in samples], np.float64),
           "shadow": np.array([s[2] for s in samples], np.uint32),
           "normal": np.array([s[3] for s in samples], np.float64).reshape(-1, 3)}
    return ref


def freeze(ref):
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check_misses(ref):
    """A miss is (-1, +inf, 0, zero normal) in the reference itself."""
    miss = ref["object"] < 0
    assert (ref["object"][miss] == -1).all()
    assert np.isposinf(ref["distance"][miss]).all() and np.isfinite(ref["distance"][~miss]).all()
    assert (ref["shadow"][miss] == 0).all()
    assert (ref["normal"][miss].view(np.uint64) == 0).all()


@functools.lru_cache(maxsize=None)
def reference(name, time, w, h):
    """The four planes of the perspective frame from the oracle, read-only."""
    from oracle import oracle as O
    sc = O.OracleScene(scene_text(name), time, w, h, max_depth=0)
    flat = sample_planes([oracle_sample(sc, x, y) for y in range(h) for x in range(w)])
    ref = {k: v.reshape((h, w) + v.shape[1:]) for k, v in flat.items()}
    ref["n_objects"], ref["n_lights"] = np.array(sc.n_objects), np.array(sc.n_lights)
    check_misses(ref)
    hit = ref["object"] >= 0
    print(f"{name} t={time} {w}x{h}: {sc.n_objects} objects / {sc.n_lights} lights, hit share {hit.mean():.3f}, "
          f"shadowed share of hits {(ref['shadow'][hit] != 0).mean():.3f}, masks {sorted(set(ref['shadow'][hit].tolist()))}, "
          f"objects visible {np.unique(ref['object'][hit]).size}")
    return freeze(ref)


@functools.lru_cache(maxsize=None)
def stereo_reference(name, time, w, h):
    """The same for a stereoscopic scene, composed as tests/stereo_refs.py composes colours: x >= w // 2 is the left
    eye's pixel x - w // 2, any other the right eye's."""
    text = scene_text(name)
    left, right = eye_centres(text, time, EYE_DISTANCE)
    ew = w // 2
    Ls, Rs = eye_oracle(text, time, ew, h, left, 0), eye_oracle(text, time, ew, h, right, 0)
    flat = sample_planes([oracle_sample(Ls, x - ew, y) if x >= ew else oracle_sample(Rs, x, y)
                          for y in range(h) for x in range(w)])
    ref = {k: v.reshape((h, w) + v.shape[1:]) for k, v in flat.items()}
    check_misses(ref)
    return freeze(ref)


@functools.lru_cache(maxsize=None)
def tracer(name, time, w, h, kind="perspective"):
    import tinyraytracerinrust_amd as T
    rt = T.RayTracer(w, h)
    rt.load_scene(scene_text(name), time, asset_dir=SCENES, camera_kind=kind,
                  eye_distance=EYE_DISTANCE if kind != "perspective" else None)
    return rt


def host(a):
    """A numpy copy of a device tensor (uint32 planes cross as their int32 bit patterns: every torch build copies
    those, strided views included)."""
    import torch
    if isinstance(a, np.ndarray):
        return a
    if a.dtype == torch.uint32:
        return a.view(torch.int32).cpu().numpy().view(np.uint32)
    return a.cpu().numpy()


def device_sentinels(rows, w, pad=0):
    """sentinel_planes on the device."""
    import torch
    as_i32 = int(np.uint32(SENTINELS["shadow"]).view(np.int32))
    return {"object": torch.full((rows, w + pad), SENTINELS["object"], dtype=torch.int32, device="cuda"),
            "distance": torch.full((rows, w + pad), SENTINELS["distance"], dtype=torch.float64, device="cuda"),
            "shadow": torch.full((rows, w + pad), as_i32, dtype=torch.int32, device="cuda").view(torch.uint32),
            "normal": torch.full((rows, w + pad, 3), SENTINELS["normal"], dtype=torch.float64, device="cuda")}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against(res, ref, label, planes=PLANES):
    diff = {k: int((np.ascontiguousarray(host(res[k])).view(np.uint8).reshape(ref[k].shape[:2] + (-1,)) !=
                    np.ascontiguousarray(ref[k]).view(np.uint8).reshape(ref[k].shape[:2] + (-1,))).any(axis=-1).sum())
            for k in planes}
    print(f"{label}: pixels that differ per plane {diff}")
    for k in planes:
        assert host(res[k]).dtype == DTYPES[k], k
        assert host(res[k]).shape == ref[k].shape, k
        assert same_bytes(res[k], ref[k]), (k, diff[k])


def sentinel_planes(rows, w, pad=0):
    """Host arrays of `rows` rows of w + pad pixels, every element a sentinel."""
    return {"object": np.full((rows, w + pad), SENTINELS["object"], np.int32),
            "distance": np.full((rows, w + pad), SENTINELS["distance"], np.float64),
            "shadow": np.full((rows, w + pad), SENTINELS["shadow"], np.uint32),
            "normal": np.full((rows, w + pad, 3), SENTINELS["normal"], np.float64)}


def untouched(a, k):
    return bool((host(a) == DTYPES[k](SENTINELS[k])).all())


def raw_planes(T, arrays):
    """rt_hit_planes over host arrays (a dict by plane name; absent = NULL)."""
    p = T._lib.rt_hit_planes()
    for k, a in arrays.items():
        setattr(p, k, a.ctypes.data)
        setattr(p, k + "_stride", a.strides[0])
    return p


# ---------------------------------------------------------------- 1. the whole frame
@pytest.mark.parametrize("name,time,w,h,n_objects,n_lights,has_miss", CASES)
def test_frame_equals_the_oracle(T, worldmap, name, time, w, h, n_objects, n_lights, has_miss):
    import torch
    ref = reference(name, time, w, h)
    hit = ref["object"] >= 0
    assert (int(ref["n_objects"]), int(ref["n_lights"])) == (n_objects, n_lights)
    assert hit.mean() >= 0.05                                            # non-vacuity, from the reference alone
    assert np.unique(ref["shadow"][hit]).size >= 2
    assert (~hit).any() == has_miss
    res = tracer(name, time, w, h).renderer.first_hits(shadow=True, normal=True)
    assert set(res) == set(PLANES)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in res.values())
    assert res["object"].dtype == torch.int32 and res["distance"].dtype == torch.float64
    assert res["shadow"].dtype == torch.uint32 and res["normal"].dtype == torch.float64
    assert tuple(res["object"].shape) == (h, w) and tuple(res["normal"].shape) == (h, w, 3)
    torch.cuda.synchronize()
    check_against(res, ref, f"{name} t={time} {w}x{h}")
    got = {k: host(v) for k, v in res.items()}
    check_misses(got)
    assert np.array_equal(got["object"] < 0, ~hit)


def test_raytracer_first_hits_is_the_whole_frame(T, worldmap):
    import torch
    res = tracer("globes", 0.0, W, H).first_hits()
    torch.cuda.synchronize()
    assert set(res) == {"object", "distance"}
    check_against(res, reference("globes", 0.0, W, H), "RayTracer.first_hits", ("object", "distance"))


# ---------------------------------------------------------------- 2. plane subsets
@pytest.mark.parametrize("name,time,w,h", [c[:4] for c in CASES[:2]])
def test_plane_subsets(T, worldmap, name, time, w, h):
    import torch
    ref = reference(name, time, w, h)
    r = tracer(name, time, w, h).renderer
    res = r.first_hits(shadow=False, normal=False)
    torch.cuda.synchronize()
    assert set(res) == {"object", "distance"}
    check_against(res, ref, f"{name}: id and distance", ("object", "distance"))
    for only in PLANES:                                     # one plane non-NULL through the raw ABI
        arrays = sentinel_planes(h, w)
        planes = raw_planes(T, {only: arrays[only]})
        assert T.lib().rt_first_hits(r.h, 0, h, ctypes.byref(planes), None) == RT_OK, only
        check_against(arrays, ref, f"{name}: {only} alone", (only,))
        for k in PLANES:
            if k != only:
                assert untouched(arrays[k], k), (only, k)
    arrays = sentinel_planes(h, w)                          # out= asks for exactly the planes it names
    res = r.first_hits(out={"object": arrays["object"], "shadow": arrays["shadow"]})
    assert res["object"] is arrays["object"] and res["shadow"] is arrays["shadow"]
    assert set(res) == {"object", "distance", "shadow"}
    torch.cuda.synchronize()
    check_against(res, ref, f"{name}: out= object and shadow", ("object", "distance", "shadow"))
    assert untouched(arrays["distance"], "distance") and untouched(arrays["normal"], "normal")
    part = r.first_hits(10, 31, shadow=True, normal=True)   # a row range: its rows
    torch.cuda.synchronize()
    check_against(part, {k: ref[k][10:31] for k in PLANES}, f"{name}: rows 10..31")


# ---------------------------------------------------------------- 3. row bands
@pytest.mark.parametrize("layout,world,band", LAYOUTS)
def test_bands_equal_the_reference_rows(T, worldmap, layout, world, band):
    from tinyraytracerinrust_amd import distributed as D
    ref = reference("globes", 0.0, W, H)
    r = tracer("globes", 0.0, W, H).renderer
    slot_rows = D.rows_per_rank(H, world, layout, band)
    owned, past = [], 0
    for rank in range(world):
        y_first, band_rows, pitch, n_bands = D.band_params(H, world, rank, layout, band)
        arrays = sentinel_planes(slot_rows, W)
        res = r.first_hits_row_bands(y_first, band_rows, pitch, n_bands, out=arrays)
        assert all(res[k] is arrays[k] for k in PLANES)
        for p in range(slot_rows):
            b, j = divmod(p, band_rows) if band_rows else (n_bands, 0)
            y = y_first + b * pitch + j
            if b < n_bands and y < H:
                owned.append(y)
                for k in PLANES:
                    assert same_bytes(arrays[k][p], ref[k][y]), (rank, p, y, k)
            else:                                   # a row at or past H, or past the rank's bands: never written
                past += 1
                for k in PLANES:
                    assert untouched(arrays[k][p], k), (rank, p, k)
    print(f"{layout} world={world} band={band}: rows left untouched {past}")
    assert sorted(owned) == list(range(H))
    assert past > 0


# ---------------------------------------------------------------- 4. strides, host and device planes
def test_padded_strides_and_mixed_pointers(T, worldmap):
    import torch
    ref = reference("globes", 0.0, W, H)
    r = tracer("globes", 0.0, W, H).renderer
    PAD = 3
    # every plane padded, all device
    dev = device_sentinels(H, W, PAD)
    res = r.first_hits(out={k: v[:, :W] for k, v in dev.items()})
    torch.cuda.synchronize()
    check_against(res, ref, "padded device planes")
    for k in PLANES:
        assert untouched(dev[k][:, W:], k), k
    # every plane padded, all host
    hst = sentinel_planes(H, W, PAD)
    res = r.first_hits(out={k: v[:, :W] for k, v in hst.items()})
    check_against(res, ref, "padded host planes")
    for k in PLANES:
        assert untouched(hst[k][:, W:], k), k
    # host and device planes mixed in one call, padded and tight
    hst = sentinel_planes(H, W, PAD)
    dev = device_sentinels(H, W, PAD)
    mixed = {"object": dev["object"][:, :W], "distance": hst["distance"][:, :W],
             "shadow": np.full((H, W), SENTINELS["shadow"], np.uint32), "normal": device_sentinels(H, W)["normal"]}
    res = r.first_hits(out=mixed)
    torch.cuda.synchronize()
    check_against(res, ref, "mixed host and device planes")
    assert untouched(hst["distance"][:, W:], "distance") and untouched(dev["object"][:, W:], "object")


# ---------------------------------------------------------------- 5. sample positions
def test_points(T, worldmap):
    from oracle import oracle as O
    ref = reference("globes", 0.0, W, H)
    rt = tracer("globes", 0.0, W, H)
    r = rt.renderer
    y = 30                                                  # a row through the spheres and their shadows
    assert np.unique(ref["object"][y]).size >= 3 and np.unique(ref["shadow"][y]).size >= 2
    xy = np.array([[float(x), float(y)] for x in range(W)])
    res = r.first_hits_points(xy, shadow=True, normal=True)
    assert set(res) == set(PLANES) and all(isinstance(v, np.ndarray) for v in res.values())
    for k in PLANES:
        assert res[k].dtype == DTYPES[k] and same_bytes(res[k], ref[k][y]), k
    res = r.first_hits_points(xy)
    assert set(res) == {"object", "distance"}
    assert same_bytes(res["object"], ref["object"][y]) and same_bytes(res["distance"], ref["distance"][y])
    # 32 fractional positions against both oracle paths
    rng = np.random.default_rng(20240607)
    frac = np.stack([rng.uniform(0.0, W - 1.0, 32), rng.uniform(0.0, H - 1.0, 32)], axis=1)
    sc = O.OracleScene(scene_text("globes"), 0.0, W, H, max_depth=0)
    want = sample_planes([oracle_sample(sc, x, yy) for x, yy in frac])
    assert (want["object"] >= 0).any() and (want["object"] < 0).any()
    res = r.first_hits_points(frac, shadow=True, normal=True)
    bad = {k: int((np.ascontiguousarray(res[k]).view(np.uint8).reshape(32, -1) !=
                   np.ascontiguousarray(want[k]).view(np.uint8).reshape(32, -1)).any(axis=1).sum()) for k in PLANES}
    print(f"32 fractional positions: samples that differ per plane {bad}")
    for k in PLANES:
        assert same_bytes(res[k], want[k]), (k, bad[k])
    # RayTracer.pick
    for x, yy in [(36, 30), (0, 0), (float(frac[0, 0]), float(frac[0, 1]))]:
        o, d = rt.pick(x, yy)
        wo, wd, _, _ = oracle_sample(sc, x, yy)
        assert isinstance(o, int) and isinstance(d, float)
        assert o == wo and np.float64(d).tobytes() == np.float64(wd).tobytes(), (x, yy)
    assert r.first_hits_points(np.zeros((0, 2)))["object"].shape == (0,)


# ---------------------------------------------------------------- 6. stereoscopic scenes
def test_stereoscopic_scene(T, worldmap):
    import torch
    w, h = 41, 21
    ref = stereo_reference("globes", 0.1, w, h)
    hit = ref["object"] >= 0
    assert hit.mean() >= 0.05 and np.unique(ref["shadow"][hit]).size >= 2 and (~hit).any()
    assert hit[:, :20].any() and hit[:, 20:40].any()        # both eyes see the scene
    r = tracer("globes", 0.1, w, h, "stereoscopic").renderer
    res = r.first_hits(shadow=True, normal=True)
    torch.cuda.synchronize()
    check_against(res, ref, f"globes t=0.1 {w}x{h} stereoscopic")
    y = 12
    pts = r.first_hits_points(np.array([[float(x), float(y)] for x in range(w)]), shadow=True, normal=True)
    for k in PLANES:
        assert same_bytes(pts[k], ref[k][y]), k


# ---------------------------------------------------------------- 7. errors
def test_argument_errors(T, worldmap):
    lib = T.lib()
    r = tracer("globes", 0.0, W, H).renderer
    arrays = sentinel_planes(8, W)
    all_planes = raw_planes(T, arrays)
    pp = ctypes.byref(all_planes)
    xy = np.array([[1.0, 2.0]])
    xp = ctypes.c_void_p(xy.ctypes.data)
    one = sentinel_planes(1, 1)
    ptrs = [ctypes.c_void_p(one[k].ctypes.data) for k in PLANES]
    # an anaglyph scene: refused by all three, nothing written
    ra = tracer("globes", 0.1, 41, 21, "anaglyph").renderer
    small = sentinel_planes(8, 41)
    sp = ctypes.byref(raw_planes(T, small))
    assert lib.rt_first_hits(ra.h, 0, 8, sp, None) == RT_ERR_UNSUPPORTED
    assert b"anaglyph" in lib.rt_last_error()
    assert lib.rt_first_hits_row_bands(ra.h, 0, 4, 8, 2, sp, None) == RT_ERR_UNSUPPORTED
    assert lib.rt_first_hits_points(ra.h, xp, 1, *ptrs, None) == RT_ERR_UNSUPPORTED
    with pytest.raises(T.RtError) as e:
        ra.first_hits()
    assert e.value.status == RT_ERR_UNSUPPORTED
    assert all(untouched(small[k], k) and untouched(one[k], k) for k in PLANES)
    # geometry, word for word rt_count_rays_row_bands'
    for zero in ((0, 0, 8, 1), (0, 8, 8, 0)):                                               # no rows: RT_OK, nothing written
        assert lib.rt_first_hits_row_bands(r.h, *zero, pp, None) == RT_OK
    assert lib.rt_first_hits(r.h, 5, 5, pp, None) == RT_OK
    assert lib.rt_first_hits_row_bands(r.h, 0, 8, 4, 2, pp, None) == RT_ERR_INVALID          # pitch < rows, several bands
    assert lib.rt_first_hits_row_bands(r.h, H, 8, 8, 1, pp, None) == RT_ERR_INVALID          # y_first >= H
    assert lib.rt_first_hits(r.h, 6, 5, pp, None) == RT_ERR_INVALID                          # y0 > y1
    assert lib.rt_first_hits(r.h, 5, H + 1, pp, None) == RT_ERR_INVALID                      # y1 > H
    # a stride below its row, one plane at a time: refused, nothing written to any plane
    rows = {"object": 4 * W, "distance": 8 * W, "shadow": 4 * W, "normal": 24 * W}
    for k in PLANES:
        short = raw_planes(T, arrays)
        setattr(short, k + "_stride", rows[k] - 4)
        assert lib.rt_first_hits(r.h, 0, 8, ctypes.byref(short), None) == RT_ERR_INVALID, k
        assert lib.rt_first_hits_row_bands(r.h, 0, 4, 4, 2, ctypes.byref(short), None) == RT_ERR_INVALID, k
    # all planes NULL, a NULL plane struct
    assert lib.rt_first_hits(r.h, 0, 8, ctypes.byref(T._lib.rt_hit_planes()), None) == RT_ERR_INVALID
    assert lib.rt_first_hits_row_bands(r.h, 0, 8, 8, 1, ctypes.byref(T._lib.rt_hit_planes()), None) == RT_ERR_INVALID
    assert lib.rt_first_hits(r.h, 0, 8, None, None) == RT_ERR_INVALID
    assert lib.rt_first_hits_points(r.h, xp, 1, None, None, None, None, None) == RT_ERR_INVALID
    assert lib.rt_first_hits_points(r.h, None, 1, *ptrs, None) == RT_ERR_INVALID
    assert all(untouched(arrays[k], k) and untouched(one[k], k) for k in PLANES)
    # no scene uploaded
    fresh = T.Renderer(0)
    assert lib.rt_first_hits(fresh.h, 0, 1, pp, None) == RT_ERR_INVALID
    assert lib.rt_first_hits_row_bands(fresh.h, 0, 1, 1, 1, pp, None) == RT_ERR_INVALID
    assert lib.rt_first_hits_points(fresh.h, xp, 1, *ptrs, None) == RT_ERR_INVALID
    fresh.free()
    assert all(untouched(arrays[k], k) for k in PLANES)
    # the wrapper: no rows is an empty result, a wrong dtype or shape is refused before any address is passed
    res = r.first_hits_row_bands(0, 8, 8, 0, shadow=True, normal=True)
    assert tuple(res["object"].shape) == (0, W) and tuple(res["normal"].shape) == (0, W, 3)
    with pytest.raises(ValueError):
        r.first_hits(out={"object": np.zeros((H, W), np.int64)})
    with pytest.raises(ValueError):
        r.first_hits(out={"distance": np.zeros((H - 1, W), np.float64)})
    with pytest.raises(ValueError):
        r.first_hits(out={"colour": np.zeros((H, W), np.int32)})


def test_shadow_bits_need_at_most_32_lights(T):
    import torch
    rt = T.RayTracer(16, 16)
    rt.add_object(rt.sphere((0.0, 0.0, 0.0), 30.0))
    for k in range(33):
        rt.add_light((-10.0 + k, 30.0, -50.0))
    r = rt.renderer
    with pytest.raises(T.RtError) as e:
        r.first_hits(shadow=True)
    assert e.value.status == RT_ERR_UNSUPPORTED
    with pytest.raises(T.RtError) as e:
        r.first_hits_points(np.array([[8.0, 8.0]]), shadow=True)
    assert e.value.status == RT_ERR_UNSUPPORTED
    res = r.first_hits(normal=True)                      # the other planes are served
    torch.cuda.synchronize()
    obj = host(res["object"])
    assert obj[8, 8] == 0 and set(np.unique(obj).tolist()) <= {-1, 0}


# ---------------------------------------------------------------- 8. no side effects
def test_first_hits_change_no_later_render(T, worldmap):
    import torch
    import tinyraytracerinrust_amd as Tm
    rt = Tm.RayTracer(W, H)                              # a renderer of its own: its launch history is this test's
    rt.load_scene(scene_text("globes"), 0.0, asset_dir=SCENES)
    r = rt.renderer
    before = r.render_rows_host(0, H)
    info = r.kernel_info()
    assert "last launch: " in info
    res = r.first_hits(shadow=True, normal=True)
    torch.cuda.synchronize()
    check_against(res, reference("globes", 0.0, W, H), "between two renders")
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]
    assert r.last_kernel_ms() > 0.0                       # the call's own launch is timed
    r.first_hits_points(np.array([[3.0, 4.0]]))
    assert r.last_kernel_ms() > 0.0
    after = r.render_rows_host(0, H)
    assert np.array_equal(before, after)
    assert r.kernel_info().split("last launch: ")[1] == info.split("last launch: ")[1]


# ---------------------------------------------------------------- 9. the headless driver
def test_cli_writes_the_four_maps(T, worldmap, tmp_path):
    ref = reference("globes", 0.0, W, H)
    out = tmp_path / "globes.png"
    maps = {k: tmp_path / f"{k}.png" for k in ("object", "depth", "normal", "shadow")}
    cmd = [sys.executable, "-m", "tinyraytracerinrust_amd", "render", os.path.join(SCENES, "globes.scene"),
           "--size", f"{W}x{H}", "-o", str(out)]
    for k, p in maps.items():
        cmd += [f"--{k}-map", str(p)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stderr.strip().splitlines()[-1])
    assert info["objects_hit"] == 6
    assert info["first_hits_ms"] > 0
    got = {k: T.read_png_rgba8(str(path)) for k, path in maps.items()}
    for k in got:
        assert got[k].shape == (H, W, 4), k
    miss = ref["object"] < 0
    assert np.array_equal(got["object"][..., 0] == 0, miss)
    want = np.where(miss, 0, (ref["object"].astype(np.int64) + 1) * 255 // 6).astype(np.uint8)
    for ch in range(3):
        assert np.array_equal(got["object"][..., ch], want)
    assert (got["depth"][..., 0][miss] == 0).all() and (got["depth"][..., 0][~miss] >= 64).all()
    assert got["depth"][..., 0].max() == 255
    assert (got["normal"][..., :3][miss] == 0).all() and (got["normal"][..., :3][~miss].max(axis=-1) > 0).all()
    seen = 2 - np.array([[bin(int(v)).count("1") for v in row] for row in ref["shadow"]])
    assert np.array_equal(got["shadow"][..., 0], np.where(miss, 0, seen * 255 // 2).astype(np.uint8))
    assert out.exists()
