"""Tile masks in the specialised row kernels (csrc/rt_tilemask.h, k_masks.hip, rt_device.h trace()): the
megakernel and the primary-ray kernel of a reflection-only scene's own program skip the objects their
tile's mask words rule out.  Masks never change an accepted hit, so every frame is RGBA8-identical with
masks on, with masks off and in the CPU oracle (raytracer.rs:132-287), and the f64 colours are
bit-identical on and off.  Scenes, sizes and band layouts are test_tile_masks_host.py's."""
import numpy as np
import pytest

from tests import tile_mask_scenes as M
from tests.conftest import SCENES, scene_text

pytestmark = pytest.mark.gpu

DEPTHS = (0, 1, 2, 10)


def _oracle(text, t, W, H, depth):
    from oracle import oracle as O
    return O.OracleScene(text, t, W, H, max_depth=depth).render(0, H)[1]


def _renderer(text, t, W, H, level=1):
    """The scene's own program loaded, the megakernel pinned (launches this small would otherwise take the
    deferred kernel, which reads no masks; max_depth 0 still takes the primary-ray kernel)."""
    import tinyraytracerinrust_amd as T
    sc = T.Scene.compile(text, t, W, H, asset_dir=SCENES)
    r = T.Renderer(0, specialize=level)
    r.set_kernel("mega")
    r.set_tile_masks(True)
    r.upload(sc)
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    return sc, r


def _rows(r, y0, y1, depth, f64=False):
    import torch
    f = r.render_rows(y0, y1, max_depth=depth, f64=f64)
    torch.cuda.synchronize()
    return f.cpu().numpy()


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(M.scenes()))
def test_masked_frames_equal_unmasked_and_oracle(worldmap, name, size):
    import torch
    W, H = size
    text, t = M.scenes()[name]
    sc, r = _renderer(text, t, W, H)
    # the kernels read masks in the reflection-only mode; three_cubes and ground_star hold a transparent
    # cube (chain mode): their launches take none, and their frames are exact all the same
    masked = "tile masks: on" if ", reflection," in r.kernel_info() else "tile masks: off"
    assert (masked == "tile masks: off") == (name in ("three_cubes", "ground_star")), r.kernel_info()
    for depth in DEPTHS:
        ref = _oracle(text, t, W, H, depth)
        r.set_tile_masks(True)                  # 2: every launch that can (these launches are too small to calibrate)
        on = _rows(r, 0, H, depth)
        info = r.kernel_info()
        want = "primary-ray (specialised)" if depth == 0 else "megakernel (specialised)"
        assert want in info and masked in info, info
        r.set_tile_masks(False)                 # the program's mask-free megakernel
        off = _rows(r, 0, H, depth)
        assert want in r.kernel_info() and "tile masks: off" in r.kernel_info(), r.kernel_info()
        assert np.array_equal(on, off), f"{name} depth {depth}: {int((on != off).sum())} channels differ on / off"
        assert np.array_equal(on, ref), f"{name} depth {depth}: {int((on != ref).sum())} channels differ from the oracle"
    # rows from a y_first that is no multiple of the tile, then each rank's cyclic bands (depth 10)
    ref = _oracle(text, t, W, H, 10)
    r.set_tile_masks(True)
    part = _rows(r, 5, H - 3, 10)
    assert masked in r.kernel_info()
    assert np.array_equal(part, ref[5:H - 3]), f"{name} rows [5, {H - 3})"
    for label, y_first, band_rows, pitch, n_bands in M.geometries(H)[1:]:
        out = torch.zeros((band_rows * n_bands, W, 4), dtype=torch.uint8, device="cuda")
        r.render_row_bands(y_first, band_rows, pitch, n_bands, out, max_depth=10)
        torch.cuda.synchronize()
        assert masked in r.kernel_info(), r.kernel_info()
        got = out.cpu().numpy()
        ys = M.frame_rows(H, y_first, band_rows, pitch, n_bands)
        keep = ys >= 0
        assert np.array_equal(got[keep], ref[ys[keep]]), f"{name} {label}"
        # the device's table for this geometry is the host's (a word FP contraction changed may only gain bits)
        dev = r.tile_masks(y_first, band_rows, pitch, n_bands)
        host, _ = sc.tile_masks(y_first, band_rows, pitch, n_bands)
        differ = int((dev != host).sum())
        print(f"{name} {W}x{H} {label}: {differ} of {host.size} mask words differ between device and host")
        assert ((dev & host) == host).all(), f"{name} {label}: a device word lacks a bit of the host's"
    dev, (host, _) = r.tile_masks(), sc.tile_masks()
    print(f"{name} {W}x{H} frame: {int((dev != host).sum())} of {host.size} mask words differ between device and host")
    assert ((dev & host) == host).all()
    r.free()


def test_f64_colours_bit_identical_on_and_off(worldmap):
    """Level 2: the f64 launches run the specialised kernels too (masked), and must give the unmasked bits."""
    W, H = M.SIZES[0]
    text, t = M.scenes()["globes"]
    sc, r = _renderer(text, t, W, H, level=2)
    for depth in DEPTHS:
        r.set_tile_masks(True)
        on = _rows(r, 0, H, depth, f64=True)
        assert "tile masks: on" in r.kernel_info() and "(specialised)" in r.kernel_info(), r.kernel_info()
        r.set_tile_masks(False)
        off = _rows(r, 0, H, depth, f64=True)
        assert on.tobytes() == off.tobytes(), f"depth {depth}"
    r.free()


def test_reupload_with_moved_object_and_camera_recomputes_the_table(worldmap):
    """Same structure, other positions: the tile order would stay, the masks must not."""
    import tinyraytracerinrust_amd as T
    W, H = M.SIZES[1]
    a = M.scenes()["cubes_csg_3lights"][0]
    b = a.replace("cube(<-30, -15, 10>, 20, red)", "cube(<12, -15, -30>, 20, red)").replace(
        "set camera(<0, 10, -85>)", "set camera(<-25, 30, -70>)")
    assert a != b
    sc, r = _renderer(a, 0.0, W, H)
    assert np.array_equal(_rows(r, 0, H, 10), _oracle(a, 0.0, W, H, 10))
    first = r.tile_masks()
    sc_b = T.Scene.compile(b, 0.0, W, H, asset_dir=SCENES)
    r.upload(sc_b)
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    got = _rows(r, 0, H, 10)
    assert "megakernel (specialised)" in r.kernel_info() and "tile masks: on" in r.kernel_info(), r.kernel_info()
    assert np.array_equal(got, _oracle(b, 0.0, W, H, 10))
    second = r.tile_masks()
    assert (first != second).any() and ((second & sc_b.tile_masks()[0]) == sc_b.tile_masks()[0]).all()
    r.free()


def test_default_takes_masks_where_the_calibration_says_they_pay(worldmap):
    """RT_OPT_TILE_MASKS 1 (the default), a frame large enough to calibrate (>= 2048 tiles): the ordered
    launches take the masked or the mask-free megakernel by the calibration's verdict, the primary-ray
    kernel always the table; exact either way, and 0 / 2 override."""
    import tinyraytracerinrust_amd as T
    W, H = 640, 360
    text, t = M.scenes()["globes"]
    sc = T.Scene.compile(text, t, W, H, asset_dir=SCENES)
    r = T.Renderer(0, specialize=1)
    r.set_kernel("mega")
    r.upload(sc)
    assert r.spec_wait(600_000)
    ref = _oracle(text, t, W, H, 10)
    seen = []
    for launch in range(3):                     # calibration (generic), then ordered
        assert np.array_equal(_rows(r, 0, H, 10), ref), r.kernel_info()
        seen.append(r.kernel_info().split("last launch: ")[1])
    assert "megakernel (specialised)" in seen[-1] and seen[-1] == seen[-2], seen
    print("default, 640x360 globes d10:", seen[-1])
    assert np.array_equal(_rows(r, 0, H, 0), _oracle(text, t, W, H, 0))
    assert np.array_equal(_rows(r, 0, H, 0), _oracle(text, t, W, H, 0))      # the ordered primary-ray launch
    assert "primary-ray (specialised); tile masks: on" in r.kernel_info(), r.kernel_info()
    for mode, want in ((2, "tile masks: on"), (0, "tile masks: off")):
        r.set_tile_masks(mode)
        assert np.array_equal(_rows(r, 0, H, 10), ref) and want in r.kernel_info(), r.kernel_info()
    r.free()


def test_family_frames_exact(worldmap):
    """spinning_globes t = 0 and t = 0.5 registered as a family: exact frames (a family program takes no masks)."""
    import tinyraytracerinrust_amd as T
    W, H = M.SIZES[0]
    text = scene_text("spinning_globes")
    T.Scene.clear_families()
    try:
        T.Scene.register_family([T.Scene.compile(text, t, W, H, asset_dir=SCENES) for t in (0.0, 0.5)])
        for t in (0.0, 0.5):
            sc, r = _renderer(text, t, W, H)
            got = _rows(r, 0, H, 10)
            assert np.array_equal(got, _oracle(text, t, W, H, 10)), f"t = {t} ({r.kernel_info()})"
            assert "tile masks: off" in r.kernel_info(), r.kernel_info()
            r.free()
    finally:
        T.Scene.clear_families()
