"""The anti-aliasing pass by row bands (rt_antialias_row_bands) and the edge overlay (rt_antialias_edges).

A band call must write exactly the rows of rt_antialias' whole-frame output that it owns -- bit for bit in RGBA8
and in f64, the arithmetic per pixel being the same -- packed as rt_render_row_bands packs a render, and count
exactly those rows' sub-pixel rays.  The source frame is always the GPU's own render, as in
tests/test_gpu_antialias.py, which isolates the pass.

Shapes: 72x53 (W no multiple of the classify kernel's 16-pixel tile, H no multiple of any band) with bands of 5
rows (no multiple of a wave's 8 rows, so tiles straddle bands; the last band is partial and owns frame row 52, the
pass-through row), of 8 rows, and contiguous thirds.  The CPU oracle has, for globes t=0 at 72x53, threshold 0.01:
713 edge pixels, none in rows 0..9, and 29 788 level-3 rays; the tests below assert what they need of that."""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9               # tests/test_gpu_antialias.py's bars: f64 within 1e-9 of the oracle, RGBA8 exact
W, H, TH, LEVEL = 72, 53, 0.01, 3
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -6
LAYOUTS = [("cyclic", 3, 5), ("cyclic", 2, 8), ("contiguous", 3, 0)]


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


class Whole:
    """One scene's renderer, its rendered frame and the whole-frame pass over it: computed once, never changed."""

    def __init__(self, T, name, time, w, h, threshold, level):
        self.rt = T.RayTracer(w, h)
        self.rt.load_scene(scene_text(name), time, asset_dir=SCENES)
        self.r = self.rt.renderer
        self.frame = self.r.render_rows_host(0, h)
        self.u8, self.rays = self.r.antialias(self.frame, threshold, level)
        self.f64, rays = self.r.antialias(self.frame, threshold, level, f64=True)
        assert rays == self.rays
        for a in (self.frame, self.u8, self.f64):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def globes(T, worldmap):
    return Whole(T, "globes", 0.0, W, H, TH, LEVEL)


def _bands(G, params, f64, rows=None, fill=0, threshold=TH, level=LEVEL):
    """One band call into a host array of `rows` rows (default: the packed rows) prefilled with `fill`."""
    n = params[1] * params[3] if rows is None else rows
    out = np.full((n, G.frame.shape[1], 4), fill, np.float64 if f64 else np.uint8)
    res, rays = G.r.antialias_row_bands(G.frame, *params, threshold, level, f64=f64, out=out)
    assert res is out
    return out, rays


def _partition(G, layout, world, band, f64, threshold=TH, level=LEVEL):
    """Every rank's band call on the one context -> (frame assembled on the CPU, per-rank rays)."""
    import torch
    from tinyraytracerinrust_amd import distributed as D
    h = G.frame.shape[0]
    slot_rows = D.rows_per_rank(h, world, layout, band)
    slots, rays = [], []
    for rank in range(world):
        out, n = _bands(G, D.band_params(h, world, rank, layout, band), f64, rows=slot_rows, threshold=threshold,
                        level=level)
        slots.append(out)
        rays.append(n)
    gathered = torch.from_numpy(np.concatenate(slots))
    return D.assemble_reference(gathered, h, world, layout, band).numpy(), rays


# ---------------------------------------------------------------- 1. a partition equals the whole frame
@pytest.mark.parametrize("f64", [False, True], ids=["rgba8", "f64"])
@pytest.mark.parametrize("layout,world,band", LAYOUTS)
def test_partition_equals_whole_frame(globes, layout, world, band, f64):
    got, rays = _partition(globes, layout, world, band, f64)
    want = globes.f64 if f64 else globes.u8
    print(f"{layout} world={world} band={band} f64={f64}: rays per rank {rays}, whole {globes.rays}")
    assert np.array_equal(got, want)                     # f64 too: the same arithmetic per pixel
    assert sum(rays) == globes.rays > 0


@pytest.mark.parametrize("f64", [False, True], ids=["rgba8", "f64"])
def test_partition_device_resident(T, globes, f64):
    """Device tensors in, the slots concatenated on the device, placed by rt_assemble_row_bands."""
    import torch
    from tinyraytracerinrust_amd import distributed as D
    layout, world, band = LAYOUTS[0]
    src = torch.from_numpy(np.array(globes.frame)).cuda()
    slot_rows = D.rows_per_rank(H, world, layout, band)
    slots, rays = [], 0
    for rank in range(world):
        slot = torch.zeros((slot_rows, W, 4), dtype=torch.float64 if f64 else torch.uint8, device=src.device)
        out, n = globes.r.antialias_row_bands(src, *D.band_params(H, world, rank, layout, band), TH, LEVEL, f64=f64,
                                              out=slot)
        assert out is slot and out.is_cuda
        slots.append(slot)
        rays += n
    frame = D.assemble(torch.cat(slots), H, world, layout, band)
    torch.cuda.synchronize()
    assert frame.is_cuda and np.array_equal(frame.cpu().numpy(), globes.f64 if f64 else globes.u8)
    assert rays == globes.rays > 0


# ---------------------------------------------------------------- 2. oracle parity of a band
@pytest.mark.parametrize("name,time,level", [("globes", 0.0, 3), ("spinning_globes", 0.3, 2)])
def test_band_oracle_parity(T, worldmap, globes, name, time, level):
    from oracle import oracle as O
    G = globes if name == "globes" else Whole(T, name, time, W, H, TH, level)
    rf, ru, rrays = O.OracleScene(scene_text(name), time, W, H, max_depth=G.rt.max_depth).antialias(G.frame, TH, level)
    gu, rays = _bands(G, (20, 20, 20, 1), False, level=level)
    gf, rays2 = _bands(G, (20, 20, 20, 1), True, level=level)
    print(f"{name} rows 20..39 level {level}: rays {rays} of the oracle's {rrays}; f64 max |d| {np.abs(gf - rf[20:40]).max():.3e}")
    assert np.array_equal(gu, ru[20:40])
    assert np.abs(gf - rf[20:40]).max() <= F64_TOL
    assert 0 < rays == rays2 <= rrays


# ---------------------------------------------------------------- 3. empty and edge cases
def test_band_without_edges(globes):
    """Rows 0..4 of the globes frame hold no edge pixel: no rays, every pixel its corners' average."""
    gf, rays = _bands(globes, (0, 5, 5, 1), True)
    gu, rays2 = _bands(globes, (0, 5, 5, 1), False)
    assert rays == rays2 == 0
    c = globes.frame.astype(np.float64) / 255.0
    avg = (((c[0:5, :-1] + c[0:5, 1:]) + c[1:6, :-1]) + c[1:6, 1:]) / 4.0      # aa_avg's order of additions
    assert np.array_equal(gf[:, :-1], avg) and np.array_equal(gf[:, -1], c[0:5, -1])
    assert np.array_equal(gf, globes.f64[0:5]) and np.array_equal(gu, globes.u8[0:5])
    assert globes.rays > 0                                                      # the frame as a whole is not edge-free


@pytest.mark.parametrize("f64", [False, True], ids=["rgba8", "f64"])
@pytest.mark.parametrize("params,frame_rows", [
    ((50, 5, 5, 1), [50, 51, 52]),                                   # one band reaching past H: 3 rows written
    ((48, 8, 8, 1), [48, 49, 50, 51, 52]),
    ((45, 5, 10, 3), [45, 46, 47, 48, 49]),                          # bands 2 and 3 start past H
    ((5, 5, 15, 4), [5, 6, 7, 8, 9, 20, 21, 22, 23, 24, 35, 36, 37, 38, 39, 50, 51, 52]),   # rank 1 of 3: last band partial
])
def test_rows_past_the_frame_are_skipped(globes, params, frame_rows, f64):
    sentinel = 171
    rows = params[1] * params[3] + 2
    out, rays = _bands(globes, params, f64, rows=rows, fill=sentinel)
    want = (globes.f64 if f64 else globes.u8)[frame_rows]
    n = len(frame_rows)
    assert np.array_equal(out[:n], want)
    assert (out[n:] == sentinel).all()                               # skipped rows and the rows beyond: untouched
    if 52 in frame_rows:
        assert np.array_equal(out[n - 1], globes.frame[52] / 255.0 if f64 else globes.frame[52])   # passed through
    assert rays > 0


def test_no_bands_writes_nothing(globes):
    for params in ((0, 5, 5, 0), (0, 0, 5, 3), (0, 0, 0, 0)):
        out = np.full((4, W, 4), 171, np.uint8)
        res, rays = globes.r.antialias_row_bands(globes.frame, *params, TH, LEVEL, out=out)
        assert rays == 0 and (out == 171).all()
    res, rays = globes.r.antialias_row_bands(globes.frame, 0, 0, 0, 0, TH, LEVEL)      # what a rank without rows gets
    assert res.shape == (0, W, 4) and rays == 0


# ---------------------------------------------------------------- 4. levels
@pytest.fixture(scope="module")
def small(T, worldmap):
    G = Whole(T, "globes", 0.0, 40, 21, TH, 4)
    G.u8_l0, G.rays_l0 = G.r.antialias(G.frame, TH, 0)
    return G


@pytest.mark.parametrize("level", [0, 4])
def test_levels(small, level):
    got, rays = _partition(small, "cyclic", 2, 3, False, level=level)
    gotf, raysf = _partition(small, "cyclic", 2, 3, True, level=level)
    if level == 0:
        assert np.array_equal(got, small.u8_l0) and sum(rays) == sum(raysf) == small.rays_l0 == 0
    else:
        assert np.array_equal(got, small.u8) and np.array_equal(gotf, small.f64)
        assert sum(rays) == sum(raysf) == small.rays > 0


# ---------------------------------------------------------------- 5. errors
def _status(T, fn):
    with pytest.raises(T.RtError) as e:
        fn()
    return e.value.status


def test_errors(T, globes):
    r, frame = globes.r, globes.frame
    assert _status(T, lambda: r.antialias_row_bands(frame, 0, 8, 4, 2, TH, LEVEL)) == RT_ERR_INVALID   # pitch < rows
    assert _status(T, lambda: r.antialias_row_bands(frame, 0, 8, 8, 1, TH, 5)) == RT_ERR_UNSUPPORTED
    assert _status(T, lambda: r.antialias_row_bands(frame, 0, 8, 8, 1, float("nan"), LEVEL)) == RT_ERR_INVALID
    assert _status(T, lambda: r.antialias_row_bands(frame, H, 8, 8, 1, TH, LEVEL)) == RT_ERR_INVALID   # as rt_render_row_bands
    out = np.zeros((8, W, 4), np.uint8)
    rays = ctypes.c_uint64(0)
    rc = T.lib().rt_antialias_row_bands(r.h, ctypes.c_void_p(frame.ctypes.data), W * 4, TH, LEVEL, -1, 0, 8, 8, 1,
                                        ctypes.c_void_p(out.ctypes.data), W * 4 - 4, None, 0, ctypes.byref(rays), None)
    assert rc == RT_ERR_INVALID and not out.any()                  # an output stride below a row
    with pytest.raises(ValueError):
        r.antialias_row_bands(frame[:-1], 0, 8, 8, 1, TH, LEVEL)      # not the whole frame
    with pytest.raises(ValueError):
        r.antialias_row_bands(frame, 0, 8, 8, 1, TH, LEVEL, f64=True, out=np.zeros((8, W, 4), np.uint8))   # dtype
    with pytest.raises(ValueError):
        r.antialias_row_bands(frame, 0, 8, 8, 1, TH, LEVEL, out=np.zeros((8, W, 8), np.uint8)[:, :, ::2])  # rows not packed
    import torch
    with pytest.raises(ValueError):
        r.antialias_edges(torch.zeros((H, W, 8), dtype=torch.uint8, device="cuda")[:, :, ::2], TH)


def test_two_eye_scene_is_unsupported(T, worldmap):
    sc = T.Scene.compile(scene_text("globes"), 0.0, 40, 21, asset_dir=SCENES)
    sc.set_camera_kind("stereoscopic", 4.0)
    r = T.Renderer(0)
    r.upload(sc)
    frame = r.render_rows_host(0, 21)
    assert _status(T, lambda: r.antialias_row_bands(frame, 0, 8, 8, 1, TH, LEVEL)) == RT_ERR_UNSUPPORTED


# ---------------------------------------------------------------- 6. edge overlay
def _edge_mask(frame, threshold):
    """mark_edge_pixels (antialiaser.rs:173-191) restated: u8 / 255.0 in float64, mean |dRGBA| > threshold."""
    c = frame.astype(np.float64) / 255.0
    c1 = c[:-1, :-1]

    def diff(c2):
        d = np.abs(c1 - c2)
        return (((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]) / 4.0 > threshold
    mask = np.zeros(frame.shape[:2], bool)
    mask[:-1, :-1] = diff(c[1:, :-1]) | diff(c[:-1, 1:]) | diff(c[1:, 1:])
    return mask


# size None: the module's 72x53 frame; 17x33: one pixel past the kernel's 16x16 tile in x and in y (the CPU oracle's
# frame: 302 edge pixels, 179 of them in rows >= 16, 2 in column 15); 16x16: exactly one tile (92 edge pixels)
@pytest.mark.parametrize("size,threshold", [pytest.param(None, 0.01, id="0.01"), pytest.param(None, 0.0, id="0.0"),
                                            pytest.param((17, 33), 0.01, id="17x33"),
                                            pytest.param((16, 16), 0.01, id="16x16")])
def test_edge_overlay(T, globes, size, threshold):
    import torch
    if size is not None:
        globes = Whole(T, "globes", 0.0, size[0], size[1], threshold, 0)
    mask = _edge_mask(globes.frame, threshold)
    mark = np.array([np.uint8(np.float64(c) * 255.0) for c in (0.6, 1.0, 1.0, 0.5)])
    assert mark.tolist() == [153, 255, 255, 127]
    overlay, n = globes.r.antialias_edges(globes.frame, threshold)
    print(f"threshold {threshold}: {n} marked pixels")
    assert n == mask.sum() > 0
    assert np.array_equal(overlay.any(axis=2), mask)                 # the marked set, exactly
    assert (overlay[mask] == mark).all() and not overlay[~mask].any()
    assert not overlay[-1].any() and not overlay[:, -1].any()
    dev, dn = globes.r.antialias_edges(torch.from_numpy(np.array(globes.frame)).cuda(), threshold)
    assert dev.is_cuda and dn == n and np.array_equal(dev.cpu().numpy(), overlay)
    if size == (17, 33):
        assert mask[16:].any() and mask[:, 15].any()                 # past the first tile row; the tile's last column
    if size is None and threshold == 0.01:
        assert n == 713 and not mask[:10].any()                      # the CPU oracle's frame: 713 edge pixels, rows 0..9 free


# ---------------------------------------------------------------- 7. Python mirror
def test_anti_alias_line_vec(T, globes):
    aa = T.AntiAliaser(globes.rt, TH, LEVEL)
    whole = aa.anti_alias_frame(globes.frame, f64=True)
    assert aa.ray_counter == globes.rays
    before, total = aa.ray_counter, 0
    for y in (0, 25, 51):
        line = aa.anti_alias_line_vec(y, globes.frame)
        assert line.shape == (W, 4) and line.dtype == np.float64
        assert np.array_equal(line, whole[y])
        _, rays = _bands(globes, (y, 1, 1, 1), True)
        total += rays
        assert aa.ray_counter == before + total
    assert total > 0                                                  # row 25 crosses the globes
    for y in (H - 1, H, -1):
        with pytest.raises(IndexError):
            aa.anti_alias_line_vec(y, globes.frame)


# ---------------------------------------------------------------- 8. the specialised trace kernel
def test_band_takes_the_specialised_trace_kernel(T, worldmap):
    """globes t=0 at 96x72 is a scene tests/test_gpu_spec_samples.py specialises too: the process compiles its
    programs once for both files (the case's time is that hipRTC compile)."""
    w, h = 96, 72
    sc = T.Scene.compile(scene_text("globes"), 0.0, w, h, asset_dir=SCENES)
    r = T.Renderer(0, specialize=1)
    r.upload(sc)
    frame = r.render_rows_host(0, h, max_depth=10)
    params = (16, 8, 24, 2)
    g = T.Renderer(0, specialize=0)                          # the generic trace kernel, pinned
    g.upload(sc)
    generic, rays_generic = g.antialias_row_bands(frame, *params, TH, LEVEL, max_depth=10)
    ginfo = g.sample_kernel_info()
    assert "aa trace: generic (RT_OPT_SPECIALIZE is off)" in ginfo and ginfo.endswith("last sample launch: aa trace"), ginfo
    before, rays_before = r.antialias_row_bands(frame, *params, TH, LEVEL, max_depth=10)   # before the wait: either kernel
    assert r.spec_wait_samples(600_000)
    info = r.sample_kernel_info()
    assert "aa trace: specialised (rt_spec_aa" in info, info
    after, rays_after = r.antialias_row_bands(frame, *params, TH, LEVEL, max_depth=10)
    info = r.sample_kernel_info()
    assert info.endswith("last sample launch: aa trace (specialised)"), info
    assert np.array_equal(after, generic) and np.array_equal(after, before)
    assert rays_after == rays_generic == rays_before > 0
    whole, _ = r.antialias(frame, TH, LEVEL, max_depth=10)
    assert np.array_equal(after, whole[[16, 17, 18, 19, 20, 21, 22, 23, 40, 41, 42, 43, 44, 45, 46, 47]])


# ---------------------------------------------------------------- 9. the CLI flag
def test_cli_render_antialias(T, worldmap, tmp_path, monkeypatch):
    """`render --antialias` on one GPU: the PNG holds Renderer.antialias' bytes of the rendered frame, and the
    JSON line reports the pass."""
    from tinyraytracerinrust_amd.__main__ import _parse, render
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    w, h = 40, 21
    png = str(tmp_path / "aa.png")
    info = render(_parse(["render", os.path.join(SCENES, "globes.scene"), "--size", f"{w}x{h}", "--antialias",
                          "--aa-level", "2", "--channels", "4", "-o", png]))
    rt = T.RayTracer(w, h)
    rt.load_scene(scene_text("globes"), 0.0, asset_dir=SCENES)
    frame = rt.renderer.render_rows_host(0, h)
    want, rays = rt.renderer.antialias(frame, 0.01, 2)
    assert not np.array_equal(want, frame) and rays > 0
    assert np.array_equal(T.read_png_rgba8(png), want)
    assert info["aa_rays"] == rays and info["antialias_ms"] > 0 and info["gpus"] == 1
    plain = render(_parse(["render", os.path.join(SCENES, "globes.scene"), "--size", f"{w}x{h}", "--channels", "4", "-o", png]))
    assert "aa_rays" not in plain and "antialias_ms" not in plain and np.array_equal(T.read_png_rgba8(png), frame)
