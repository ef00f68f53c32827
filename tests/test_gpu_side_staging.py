"""The side entries' host-or-device staging (rt_ctx.h Stager) where no other suite compares a host plane with a
device plane of the same call: rt_render_ortho, rt_antialias_edges and rt_render_points_f64, and one band layout that
the host clamp (launch_plan.h clamp_bands) cuts, through every entry that takes one.  Every check is an equality of
bytes between two calls of the same context, and each case asserts from its own data that it is not vacuous.

The frame is 41x21 globes: 41 = 5 tiles + 1 column, 21 = 2 tile rows + 5 rows of the 8x8 tiles, and no whole
second 16x16 block of the ortho and edge kernels in either direction."""
import ctypes

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text

pytestmark = pytest.mark.gpu

W, H = 41, 21
TH, LEVEL = 0.01, 2
PAD = 3                                     # pixels of row padding in the device planes
# (y_first, band_rows, band_pitch, n_bands) on H = 21: bands at 3, 11, 19, 27, 35 -- three start below H, the last
# keeps 2 of its 4 rows: 10 packed rows of the 20 the caller laid out
CUT = (3, 4, 8, 5)
CUT_ROWS = [3, 4, 5, 6, 11, 12, 13, 14, 19, 20]


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


@pytest.fixture(scope="module")
def globes(T, worldmap):
    """(renderer, the rendered quantised frame, read-only)"""
    rt = T.RayTracer(W, H)
    rt.load_scene(scene_text("globes"), 0.0, asset_dir=SCENES)
    r = rt.renderer
    frame = r.render_rows_host(0, H)
    frame.setflags(write=False)
    return r, frame


def _addr(a):
    """(address, row stride in bytes); None: a plane not asked for."""
    if a is None:
        return None, 0
    if isinstance(a, np.ndarray):
        return a.ctypes.data, a.strides[0]
    return a.data_ptr(), a.stride(0) * a.element_size()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _padded(n, fill, dtype):
    """A device plane of n rows of W pixels inside rows of W + PAD: (the whole allocation, the plane)."""
    import torch
    big = torch.full((n, W + PAD, 4), fill, dtype=dtype, device="cuda")
    return big, big[:, :W]


def test_ortho_host_and_padded_device_rows(T, globes):
    """rt_render_ortho, rows [3, 21), both outputs of one call: numpy planes and device planes whose rows are padded
    by 3 pixels hold the same bytes, and the padding keeps its fill."""
    import torch
    r, _ = globes
    ax = T.OrthoAxes.from_area("top")
    y0, y1 = 3, H

    def ortho(u8, f64):
        (p8, s8), (pf, sf) = _addr(u8), _addr(f64)
        rc = T.lib().rt_render_ortho(r.h, ax.axis1, ax.axis2, float(ax.dir1), float(ax.dir2), float(ax.scale), y0, y1,
                                     ctypes.c_void_p(p8), s8, ctypes.c_void_p(pf), sf, ctypes.c_void_p(_stream()))
        assert rc == 0, T.lib().rt_last_error()

    h8, hf = np.full((y1 - y0, W, 4), 0xA5, np.uint8), np.full((y1 - y0, W, 4), -2.5, np.float64)
    ortho(h8, hf)
    big8, d8 = _padded(y1 - y0, 0xA5, torch.uint8)
    bigf, df = _padded(y1 - y0, -2.5, torch.float64)
    ortho(d8, df)
    torch.cuda.synchronize()
    px = h8.view(np.uint32)
    assert np.unique(px).size >= 2 and not (px == 0xA5A5A5A5).any()     # a picture (floor and globes), not the fill
    assert np.unique(hf).size >= 2 and not (hf == -2.5).any()
    assert d8.cpu().numpy().tobytes() == h8.tobytes()
    assert df.cpu().numpy().tobytes() == hf.tobytes()
    assert (big8[:, W:] == 0xA5).all() and (bigf[:, W:] == -2.5).all()
    for f64 in (False, True):                                           # and each output alone, as the wrapper asks
        assert r.render_ortho(ax, y0, y1, f64=f64).tobytes() == (hf if f64 else h8).tobytes()


def test_edges_host_and_device_frame(T, globes):
    """rt_antialias_edges over a numpy frame and over the same frame on the device: equal overlays, equal counts."""
    import torch
    r, frame = globes
    h_over, h_n = r.antialias_edges(frame, TH)
    d_over, d_n = r.antialias_edges(torch.from_numpy(frame.copy()).cuda(), TH)
    assert 0 < h_n < W * H and d_n == h_n
    assert isinstance(h_over, np.ndarray) and d_over.is_cuda
    assert d_over.cpu().numpy().tobytes() == h_over.tobytes()
    assert np.unique(h_over.view(np.uint32)).size >= 2                  # marked and unmarked pixels


@pytest.mark.parametrize("dev_in", [False, True])
@pytest.mark.parametrize("dev_out", [False, True])
def test_points_host_and_device(T, globes, dev_in, dev_out):
    """rt_render_points_f64 at 70 positions (more than a wave, less than a 256-thread block): every combination of
    host and device input and output gives the wrapper's (host, host) bytes."""
    import torch
    r, _ = globes
    rng = np.random.default_rng(22)
    xy = np.ascontiguousarray(rng.uniform((0.0, 0.0), (W, H), (70, 2)))
    ref = r.render_points(xy)
    assert np.unique(ref, axis=0).shape[0] > 10
    src = torch.from_numpy(xy).cuda() if dev_in else xy
    out = torch.full((70, 4), -2.5, dtype=torch.float64, device="cuda") if dev_out else np.full((70, 4), -2.5)
    rc = T.lib().rt_render_points_f64(r.h, ctypes.c_void_p(_addr(src)[0]), 70, -1, ctypes.c_void_p(_addr(out)[0]),
                                      ctypes.c_void_p(_stream()))
    assert rc == 0, T.lib().rt_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy() if dev_out else out
    assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("device", [False, True])
def test_cut_band_layout(T, globes, device):
    """A layout the clamp cuts (five bands asked for, three start inside the frame, the last keeps two rows), through
    first_hits_row_bands, count_rays_row_bands and antialias_row_bands: the 10 packed rows equal the same rows of
    the whole-frame call, and rows 10 and up of the caller's 20-row planes keep their fill."""
    import torch
    r, frame = globes
    n_all, n = CUT[1] * CUT[3], len(CUT_ROWS)
    assert n_all == 20 and n == 10

    def plane(shape, dtype, fill):
        a = np.full((n_all,) + shape, fill, dtype)
        if not device:
            return a
        if dtype == np.uint32:                                          # (torch copies no uint32 from numpy)
            return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)
        return torch.from_numpy(a).cuda()

    def host(a):
        if isinstance(a, np.ndarray):
            return a
        torch.cuda.synchronize()
        if a.dtype == torch.uint32:
            return a.view(torch.int32).cpu().numpy().view(np.uint32)
        return a.cpu().numpy()

    def check(got, whole, fill):
        got, whole = host(got), host(whole)
        assert got[:n].tobytes() == np.ascontiguousarray(whole[CUT_ROWS]).tobytes()
        assert (got[n:] == fill).all()

    # first hits: all four planes
    whole = r.first_hits(shadow=True, normal=True, out={k: np.zeros((H, W) + s, d) for k, d, s in
                                                       (("object", np.int32, ()), ("distance", np.float64, ()),
                                                        ("shadow", np.uint32, ()), ("normal", np.float64, (3,)))})
    assert (whole["object"][CUT_ROWS] >= 0).any() and (whole["object"][CUT_ROWS] < 0).any()
    out = {"object": plane((W,), np.int32, -7), "distance": plane((W,), np.float64, -1.5),
           "shadow": plane((W,), np.uint32, 0xDEADBEEF), "normal": plane((W, 3), np.float64, -2.5)}
    got = r.first_hits_row_bands(*CUT, out=out)
    for k, fill in (("object", -7), ("distance", -1.5), ("shadow", 0xDEADBEEF), ("normal", -2.5)):
        check(got[k], whole[k], fill)
    # ray counts: totals, row sums, pixel counts
    whole = r.count_rays(rows=True, pixels=True)
    got = r.count_rays_row_bands(*CUT, out_rows=plane((4,), np.uint64 if not device else np.int64, 77),
                                 out_pixels=plane((W, 4), np.uint32 if not device else np.int32, 77))
    check(got["rows"], whole["rows"].astype(host(got["rows"]).dtype), 77)
    check(got["pixels"], whole["pixels"].astype(host(got["pixels"]).dtype), 77)
    sums = whole["rows"][CUT_ROWS].sum(axis=0)
    assert [got[k] for k in ("primary", "shadow", "reflect", "refract")] == [int(v) for v in sums] and sums[2] > 0
    # anti-aliasing: both formats
    for f64 in (False, True):
        whole, _ = r.antialias(frame, TH, LEVEL, f64=f64)
        src = torch.from_numpy(frame.copy()).cuda() if device else frame
        got, rays = r.antialias_row_bands(src, *CUT, TH, LEVEL, f64=f64,
                                          out=plane((W, 4), np.float64 if f64 else np.uint8, 0xA5))
        assert rays > 0
        check(got, whole, 0xA5)
