"""The sample programs on the GPU (tinyraytracerinrust_amd/csrc/spec_text.cpp rt_spec_points / rt_spec_aa,
RT_OPT_SPEC_SAMPLES): rt_render_points_f64 and the anti-aliasing trace through the scene-specialised device
code -- the unrolled walks over literal f32 boxes and the inlined texel guard the full frames render with.

The adversarial points of tests/test_gpu_cull_edges.py (silhouettes and shadow edges, bisected to adjacent
doubles) and of tests/test_gpu_texel_boundary.py (texel-coordinate crossings) go through the specialised
points kernel here, and through the generic one on a second renderer; the anti-aliasing pass through the
specialised trace kernel.  The bars are the project's: RGBA8 equal to the oracle's, f64 within 1e-9.  Every
case also pins WHICH kernel ran (rt_ctx_sample_kernel_info), and the lifetime cases pin that no call ever
launches a previous scene's kernel and that the row programs do not notice the sample programs.

Frames are 160x120 or smaller; a case's time is the hipRTC compile of its scene's programs (seconds, once per
scene and process: the process cache serves the later cases)."""
import math
import re

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.test_gpu_cull_edges import CUBES, _edges, _u8

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
WAIT_MS = 600_000
DEPTH = 10


def _text(name):
    if name == "cubes":
        return CUBES
    if name == "fuzz7774":
        from tests.scene_fuzz import random_scene
        return random_scene(7774)
    return scene_text(name)


def _renderer(T, text, t, W, H, specialize, kind=None, eye_distance=0.0):
    sc = T.Scene.compile(text, t, W, H, asset_dir=SCENES)
    assert sc.status == 0, sc.error
    if kind:
        sc.set_camera_kind(kind, eye_distance)
    r = T.Renderer(0, specialize=specialize)
    r.upload(sc)
    return r


def _ring(lo, hi):
    """The 8 doubles around an adjacent pair: 3 more on each side."""
    ring = [lo, hi]
    for _ in range(3):
        ring = [math.nextafter(ring[0], -math.inf)] + ring + [math.nextafter(ring[-1], math.inf)]
    return ring


def _check_points(gpu, ref, pts, label):
    g8, r8 = _u8(gpu[:, :3]), _u8(ref[:, :3])
    bad = np.nonzero((g8 != r8).any(axis=1))[0]
    d = np.abs(gpu - ref)
    print(f"{label}: {len(pts)} points, f64 bit-equal {100 * np.mean((gpu == ref).all(axis=1)):.2f} %, "
          f"max |d| {np.nanmax(d):.3e}, RGBA8 mismatches {len(bad)}")
    assert len(bad) == 0, [(pts[i], g8[i].tolist(), r8[i].tolist()) for i in bad[:8]]
    assert np.array_equal(np.isnan(gpu), np.isnan(ref)) and np.nanmax(d) <= F64_TOL
    assert (gpu[:, 3] == 1.0).all()


def _both_renderers(T, text, t, W, H, pts, ref, label):
    """The points through the specialised kernel, then through the generic one of a specialize=0 renderer."""
    xy = np.array(pts, dtype=np.float64)
    r = _renderer(T, text, t, W, H, 1)
    assert r.spec_wait_samples(WAIT_MS)
    gpu = r.render_points(xy, max_depth=DEPTH)
    info = r.sample_kernel_info()
    print(info)
    assert "last sample launch: points (specialised)" in info, info
    assert "points: specialised (rt_spec_points" in info, info
    _check_points(gpu, ref, pts, label + " specialised")
    g = _renderer(T, text, t, W, H, 0)
    gen = g.render_points(xy, max_depth=DEPTH)
    ginfo = g.sample_kernel_info()
    assert ginfo.endswith("last sample launch: points") and "points: generic (RT_OPT_SPECIALIZE is off)" in ginfo, ginfo
    _check_points(gen, ref, pts, label + " generic")


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


# ---------------------------------------------------------------- 1. edges through the specialised points kernel
@pytest.mark.parametrize("name,t,min_edges", [
    ("globes", 0.0, 50), ("cubes", 0.0, 50), ("spinning_globes", 0.5, 50), ("three_cubes", 0.0, 50),
    ("ground_star", 0.2, 50), ("fuzz7774", 0.0, 30),       # reflection, chain (spinning_globes) and ray-tree (fuzz) programs
])
def test_edges_through_the_specialised_points_kernel(T, worldmap, name, t, min_edges):
    from oracle import oracle as O
    W, H = 160, 120
    text = _text(name)
    osc = O.OracleScene(text, t, W, H, max_depth=DEPTH)
    pts = []
    for along_x in (True, False):
        for lo, hi, c in _edges(osc, W, H, along_x, n_lines=12, step=1.0, cap=60):
            pts += [(v, c) if along_x else (c, v) for v in _ring(lo, hi)]
    assert len(pts) >= 8 * min_edges, len(pts)
    ref = np.array([osc.get_pixel(x, y) for x, y in pts])
    _both_renderers(T, text, t, W, H, pts, ref, f"{name} edges")


# ---------------------------------------------------------------- 2. texel boundaries through it
def _crossings(osc, along_x, k, lines, t0, t1, step, cap):
    """tests/test_gpu_texel_boundary.py _crossings with its ranges as parameters: pairs (lo, hi, c) of adjacent
    doubles along scan line c where coordinate k of the texel lookup (0: x, 1: y) changes its integer part."""
    pairs = []
    per_line = -(-cap // len(lines))
    for c in lines:
        prev, n0 = None, len(pairs)
        for t in np.arange(t0, t1, step):
            x, y = (t, c) if along_x else (c, t)
            o, tx = osc.texel_probe(x, y)
            cur = (t, math.floor(tx[k])) if o >= 0 else None
            if prev and cur and prev[1] != cur[1]:
                lo, hi, f0 = prev[0], cur[0], prev[1]
                while math.nextafter(lo, hi) != hi:          # bisect to adjacent doubles
                    mid = 0.5 * (lo + hi)
                    if mid == lo or mid == hi:
                        break
                    xm, ym = (mid, c) if along_x else (c, mid)
                    om, tm = osc.texel_probe(xm, ym)
                    if om < 0:
                        break
                    if math.floor(tm[k]) == f0:
                        lo = mid
                    else:
                        hi = mid
                if math.nextafter(lo, hi) == hi:
                    pairs.append((lo, hi, c))
                    if len(pairs) >= cap:
                        return pairs
                    if len(pairs) - n0 >= per_line:
                        break
            prev = cur
    return pairs


def test_texel_boundaries_through_the_specialised_points_kernel(T, worldmap):
    from oracle import oracle as O
    W, H = 160, 120                                           # the textured globe covers x 58-100, y 32-72
    text = scene_text("globes")
    osc = O.OracleScene(text, 0.0, W, H, max_depth=DEPTH)
    pts = []
    for lo, hi, c in _crossings(osc, True, 0, np.linspace(36, 68, 8), 58.0, 101.0, 0.37, 40):
        pts += [(v, c) for v in _ring(lo, hi)]
    for lo, hi, c in _crossings(osc, False, 1, np.linspace(62, 96, 8), 32.0, 73.0, 0.37, 40):
        pts += [(c, v) for v in _ring(lo, hi)]
    assert len(pts) >= 8 * 60, len(pts)
    ref = np.array([osc.get_pixel(x, y) for x, y in pts])
    _both_renderers(T, text, 0.0, W, H, pts, ref, "globes texel boundaries")


# ---------------------------------------------------------------- 3. anti-aliasing
@pytest.mark.parametrize("name,t,W,H,threshold,level", [
    ("globes", 0.0, 96, 72, 0.01, 3), ("spinning_globes", 0.3, 96, 72, 0.01, 3), ("three_cubes", 0.0, 96, 72, 0.01, 3),
    ("globes", 0.0, 64, 48, 0.0, 2),
])
def test_antialias_through_the_specialised_trace_kernel(T, worldmap, name, t, W, H, threshold, level):
    import torch
    from oracle import oracle as O
    text = scene_text(name)
    r = _renderer(T, text, t, W, H, 1)
    assert r.spec_wait_samples(WAIT_MS)
    frame = r.render_rows_host(0, H, max_depth=DEPTH)
    rf, ru, rrays = O.OracleScene(text, t, W, H, max_depth=DEPTH).antialias(frame, threshold, level)
    gf, grays = r.antialias(frame, threshold, level, max_depth=DEPTH, f64=True)          # host arrays
    info = r.sample_kernel_info()
    assert "last sample launch: aa trace (specialised)" in info and "aa trace: specialised (rt_spec_aa" in info, info
    gu, grays2 = r.antialias(frame, threshold, level, max_depth=DEPTH)
    dev = torch.from_numpy(frame).cuda()                                                   # device tensors
    df, drays = r.antialias(dev, threshold, level, max_depth=DEPTH, f64=True)
    du, drays2 = r.antialias(dev, threshold, level, max_depth=DEPTH)
    torch.cuda.synchronize()
    assert r.sample_kernel_info().endswith("last sample launch: aa trace (specialised)")
    print(f"{name} {W}x{H} th={threshold} level={level}: rays gpu={grays} oracle={rrays}; f64 max |d| {np.abs(gf - rf).max():.3e}")
    assert grays == grays2 == drays == drays2 == rrays > 0
    for f64, u8 in ((gf, gu), (df.cpu().numpy(), du.cpu().numpy())):
        assert np.abs(f64 - rf).max() <= F64_TOL
        assert np.array_equal(u8, ru)
        assert np.array_equal(u8[-1], frame[-1]) and np.array_equal(u8[:, -1], frame[:, -1])   # last row and column untouched


# ---------------------------------------------------------------- 4. lifetime
def _grid_points(W, H, n, seed):
    rng = np.random.default_rng(seed)
    return [(float(x), float(y)) for x, y in zip(rng.uniform(0.0, W - 1.0, n), rng.uniform(0.0, H - 1.0, n))]


def _hash(info, path):
    m = re.search(path + r": specialised \(\w+ of hipRTC ([0-9a-f]{16})", info)
    assert m, info
    return m.group(1)


def test_upload_never_launches_the_previous_scenes_kernel(T, worldmap):
    from oracle import oracle as O
    W, H = 160, 120
    a_text, b_text = scene_text("globes"), scene_text("three_cubes")
    A = T.Scene.compile(a_text, 0.0, W, H, asset_dir=SCENES)
    B = T.Scene.compile(b_text, 0.0, W, H, asset_dir=SCENES)
    pts = _grid_points(W, H, 200, 1)
    xy = np.array(pts)
    ref_a = np.array([O.OracleScene(a_text, 0.0, W, H, max_depth=DEPTH).get_pixel(x, y) for x, y in pts])
    ref_b = np.array([O.OracleScene(b_text, 0.0, W, H, max_depth=DEPTH).get_pixel(x, y) for x, y in pts])
    r = T.Renderer(0, specialize=1)
    r.upload(A)
    assert r.spec_wait_samples(WAIT_MS)
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_a, pts, "A")
    info_a = r.sample_kernel_info()
    hash_a = _hash(info_a, "points")
    assert _hash(info_a, "aa trace") == hash_a and info_a.endswith("points (specialised)")
    r.upload(B)                                              # different geometry: A's modules are unloaded
    assert hash_a not in r.sample_kernel_info()
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_b, pts, "B, the very next call")
    assert hash_a not in r.sample_kernel_info()
    assert r.spec_wait_samples(WAIT_MS)                      # a context that asked once requests them with every upload
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_b, pts, "B specialised")
    info_b = r.sample_kernel_info()
    assert info_b.endswith("points (specialised)") and hash_a not in info_b and _hash(info_b, "points") != hash_a
    r.upload(A)                                              # A again: no fresh compile
    assert r.spec_wait_samples(WAIT_MS)
    info = r.sample_kernel_info()
    assert _hash(info, "points") == hash_a and info.count("[process cache]") == 2, info
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_a, pts, "A again")
    assert r.sample_kernel_info().endswith("points (specialised)")
    r.set_spec_samples(False)
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_a, pts, "A, option off")
    info = r.sample_kernel_info()
    assert info.endswith("last sample launch: points") and "points: generic (RT_OPT_SPEC_SAMPLES is off)" in info, info
    r.set_spec_samples(True)
    _check_points(r.render_points(xy, max_depth=DEPTH), ref_a, pts, "A, option on again")
    assert r.sample_kernel_info().endswith("points (specialised)")


def test_large_scene_keeps_the_generic_sample_kernels(T, worldmap):
    from oracle import oracle as O
    W, H = 64, 48
    text = scene_text("fractal")
    r = _renderer(T, text, 0.0, W, H, 1)
    assert r.spec_wait_samples(WAIT_MS)                      # nothing to wait for
    pts = _grid_points(W, H, 200, 2)
    osc = O.OracleScene(text, 0.0, W, H, max_depth=DEPTH)
    ref = np.array([osc.get_pixel(x, y) for x, y in pts])
    _check_points(r.render_points(np.array(pts), max_depth=DEPTH), ref, pts, "fractal")
    info = r.sample_kernel_info()
    assert "points: generic (scene too large" in info and "aa trace: generic (scene too large" in info, info
    assert info.endswith("last sample launch: points")


def test_two_eye_scene_keeps_the_generic_sample_kernels(T, worldmap):
    from tests.stereo_refs import EYE_DISTANCE, point_reference
    W, H = 40, 24
    pts = [(0.0, 0.0), (12.25, 9.5), (19.5, 12.0), (27.75, 15.125), (39.5, 23.5), (20.0, 20.0)]
    want = point_reference("globes", 0.1, W, H, DEPTH, "anaglyph", pts)
    r = _renderer(T, scene_text("globes"), 0.1, W, H, 1, "anaglyph", EYE_DISTANCE)
    assert r.spec_wait_samples(WAIT_MS)
    got = r.render_points(np.array(pts), max_depth=DEPTH)
    assert np.max(np.abs(got - want)) <= F64_TOL and (got[:, 3] == 1.0).all()
    info = r.sample_kernel_info()
    assert "points: generic (two-eye scene" in info and info.endswith("last sample launch: points"), info


# ---------------------------------------------------------------- 5. the row programs do not notice
def test_rows_untouched_by_the_sample_programs(T, worldmap):
    from oracle import oracle as O
    W, H = 160, 120
    text = scene_text("globes")
    _, ref = O.OracleScene(text, 0.0, W, H, max_depth=DEPTH).render(0, H)
    r = _renderer(T, text, 0.0, W, H, 1)
    assert r.spec_wait(WAIT_MS)                              # the row programs alone: no sample job exists yet
    assert "not requested yet" in r.sample_kernel_info()
    frames = [r.render_rows_host(0, H, max_depth=DEPTH) for _ in range(2)]
    info0 = r.kernel_info()
    assert "(specialised)" in info0
    assert r.spec_wait_samples(WAIT_MS)
    r.render_points(np.array(_grid_points(W, H, 64, 3)), max_depth=DEPTH)
    assert r.sample_kernel_info().endswith("points (specialised)")
    frames.append(r.render_rows_host(0, H, max_depth=DEPTH))
    assert r.kernel_info() == info0                          # character for character
    for f in frames:
        assert np.array_equal(f, ref)
    # a context that keeps asking: after the next upload spec_wait returns with the row programs, whatever the
    # sample jobs (queued behind them) are doing, and the sample programs arrive on their own
    r.upload(T.Scene.compile("draw(sphere(<3, 1, 2>, 27.5, red))\ndraw(sphere(<-40, 5, 20>, 12, blue, 0.4))", 0.0, W, H))
    assert r.spec_wait(WAIT_MS) and r.kernel_variant() == "spec"
    during = r.sample_kernel_info()
    print("after spec_wait:", during)
    assert "not requested yet" not in during                 # requested by the upload itself
    assert r.spec_wait_samples(WAIT_MS)
    assert "points: specialised" in r.sample_kernel_info() and "aa trace: specialised" in r.sample_kernel_info()


# ---------------------------------------------------------------- 6. one family case
def test_family_member_points_and_antialias(T, worldmap):
    from oracle import oracle as O
    W, H = 96, 72
    text = scene_text("spinning_globes")
    times = [f / 12 for f in range(4)]
    scenes = [T.Scene.compile(text, t, W, H, asset_dir=SCENES) for t in times]
    T.Scene.clear_families()
    try:
        T.Scene.register_family(scenes)
        members = [i for i, s in enumerate(scenes) if "#define RT_SPEC_FAMILY 1" in s.spec_program()]
        assert members, "no frame is in a family of several"
        i = members[-1]
        r = T.Renderer(0, specialize=1)
        r.upload(scenes[i])
        assert r.spec_wait(WAIT_MS) and "family of" in r.kernel_info(), r.kernel_info()
        assert r.spec_wait_samples(WAIT_MS)
        osc = O.OracleScene(text, times[i], W, H, max_depth=DEPTH)
        pts = _grid_points(W, H, 200, 4)
        ref = np.array([osc.get_pixel(x, y) for x, y in pts])
        _check_points(r.render_points(np.array(pts), max_depth=DEPTH), ref, pts, f"family member {i}")
        assert r.sample_kernel_info().endswith("points (specialised)"), r.sample_kernel_info()
        frame = r.render_rows_host(0, H, max_depth=DEPTH)
        rf, ru, rrays = osc.antialias(frame, 0.01, 2)
        gf, grays = r.antialias(frame, 0.01, 2, max_depth=DEPTH, f64=True)
        gu, _ = r.antialias(frame, 0.01, 2, max_depth=DEPTH)
        assert r.sample_kernel_info().endswith("aa trace (specialised)"), r.sample_kernel_info()
        assert grays == rrays > 0 and np.abs(gf - rf).max() <= F64_TOL and np.array_equal(gu, ru)
    finally:
        T.Scene.clear_families()
