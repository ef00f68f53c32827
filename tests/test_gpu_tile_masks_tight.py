"""The tighter tile-mask predicate on the device (csrc/rt_tilemask.h through k_masks.hip tile_masks_kernel):
the device's table is the host's word for word on the one-object scenes of tile_mask_tight_scenes.py (vertex
sets, ball and clip are plain f64 without contraction or a square root, so not one word may differ), and a
specialised program that reads such a table renders the oracle's frame, masks on and off."""
import numpy as np
import pytest

from tests import tile_mask_scenes as M
from tests import tile_mask_tight_scenes as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_table_equals_host(size):
    """Every scene, the whole frame and each rank's cyclic bands; no program is compiled (the table is the
    upload's, not the program's)."""
    import tinyraytracerinrust_amd as T
    W, H = size
    r = T.Renderer(0, specialize=0)
    for name, text in sorted(X.scenes().items()):
        sc = T.Scene.compile(text, 0.0, W, H)
        r.upload(sc)
        for label, y_first, band_rows, pitch, n_bands in M.geometries(H):
            dev = r.tile_masks(y_first, band_rows, pitch, n_bands)
            host, info = sc.tile_masks(y_first, band_rows, pitch, n_bands)
            assert info["valid"] and (host[:, 0] != 0xFFFFFFFF).any()
            differ = int((dev != host).sum())
            assert differ == 0, f"{name} {W}x{H} {label}: {differ} of {host.size} mask words differ between device and host"
    r.free()


@pytest.fixture(scope="module")
def rod():
    """One program for the module: the tilted rod with the light lower than its top, 100x75 (a partial tile
    column and row), the megakernel pinned and masks forced (frames this small otherwise take neither)."""
    import tinyraytracerinrust_amd as T
    W, H = X.SIZES[1]
    text = X.scenes()["rod-low_above_beside"]
    sc = T.Scene.compile(text, 0.0, W, H)
    r = T.Renderer(0, specialize=2)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    r.upload(sc)
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    yield text, W, H, sc, r
    r.free()


@pytest.mark.parametrize("depth", (0, 2))
def test_masked_frames_equal_unmasked_and_oracle(rod, depth):
    import torch
    from oracle import oracle as O
    text, W, H, sc, r = rod
    ref = O.OracleScene(text, 0.0, W, H, max_depth=depth).render(0, H)[1]
    got = {}
    for mode in (2, 0):
        r.set_tile_masks(mode)
        out = torch.full((H, W, 4), 0xAB, dtype=torch.uint8, device="cuda")
        r.render_rows(0, H, max_depth=depth, out=out)
        torch.cuda.synchronize()
        assert ("tile masks: on" if mode else "tile masks: off") in r.kernel_info(), r.kernel_info()
        got[mode] = out.cpu().numpy()
        f64 = r.render_rows(0, H, max_depth=depth, f64=True)
        torch.cuda.synchronize()
        got[mode, "f64"] = f64.cpu().numpy().tobytes()
    assert np.array_equal(got[2], got[0]), f"depth {depth}: {int((got[2] != got[0]).sum())} channels differ on / off"
    assert np.array_equal(got[2], ref), f"depth {depth}: {int((got[2] != ref).sum())} channels differ from the oracle"
    assert got[2, "f64"] == got[0, "f64"], f"depth {depth}: f64 rows differ on / off"
