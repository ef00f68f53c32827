"""Dispatch records of the masked specialised row kernels (csrc/rt_blob.h RtTileRec, k_masks.hip
tile_records_kernel, rt_device.h rows_entry; RT_OPT_TILE_RECORDS): one record per order entry carries the
tile's first pixel and its mask words, gathered on the device from the geometry's mask table and the
launch's tile order.  Records only move bytes, so every frame is RGBA8-identical to the CPU oracle
(raytracer.rs:132-287) with records on and off -- for a calibrating launch (identity records), for ordered
launches, for launches too small to order, for row ranges and cyclic bands, after a same-structure upload
(the order stays, the masks and with them the records must not) and for two streams racing for a new
table.  The record's mask words reach every light's shadow walk as scalars (scenes of 1, 2, 3 and 5 lights),
and the f64 rows stay bit-identical.  Scenes and band layouts are tile_mask_scenes'."""
import functools

import numpy as np
import pytest

from tests import tile_mask_scenes as M
from tests.conftest import SCENES

pytestmark = pytest.mark.gpu

BIG = (371, 357)        # 47 x 45 = 2115 tiles: >= RT_ORDER_MIN_TILES (a calibrated order), not a multiple of 8 (the
                        # XCDs' shares differ), neither side a multiple of the tile
CHAIN_SCENES = ("three_cubes", "ground_star")     # a transparent cube: chain mode, no masks, no records


@functools.lru_cache(maxsize=None)
def _oracle_frame(key, W, H, depth):
    from oracle import oracle as O
    text, t = key if isinstance(key, tuple) else M.scenes()[key]
    return O.OracleScene(text, t, W, H, max_depth=depth).render(0, H)[1]


def _renderer(text, t, W, H, level=1, kernel="mega"):
    import tinyraytracerinrust_amd as T
    sc = T.Scene.compile(text, t, W, H, asset_dir=SCENES)
    r = T.Renderer(0, specialize=level)
    r.set_kernel(kernel)
    r.set_tile_masks(True)                      # 2: every launch that can
    r.upload(sc)
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    return sc, r


def _rows(r, y0, y1, depth, f64=False, stream=None):
    import torch
    f = r.render_rows(y0, y1, max_depth=depth, f64=f64, stream=stream)
    torch.cuda.synchronize()
    return f.cpu().numpy()


def _expect(r, kernel, records, masks=True):
    info = r.kernel_info()
    want = f"last launch: {kernel}; tile masks: {'on' if masks else 'off'}; tile records: {'on' if records else 'off'}"
    assert info.endswith(want), (want, info)


def test_calibrating_size_calibration_and_ordered_launches(worldmap):
    """Level 2, kernel choice left to the library: the calibration launch runs the program's calibrating
    kernels on identity records, the ordered launches on the order's records."""
    W, H = BIG
    text, t = M.scenes()["globes"]
    sc, r = _renderer(text, t, W, H, level=2, kernel="auto")
    frames = {}
    for depth, kernel in ((10, "megakernel (specialised)"), (0, "primary-ray (specialised)")):
        ref = _oracle_frame("globes", W, H, depth)
        for launch in ("calibration", "first ordered", "second ordered"):
            got = _rows(r, 0, H, depth)
            _expect(r, kernel, records=True)
            assert np.array_equal(got, ref), f"depth {depth}, {launch} launch: {int((got != ref).sum())} channels differ"
        frames[depth] = got
    r.set_tile_records(False)
    for depth, kernel in ((10, "megakernel (specialised)"), (0, "primary-ray (specialised)")):
        off = _rows(r, 0, H, depth)
        _expect(r, kernel, records=False)
        assert off.tobytes() == frames[depth].tobytes(), f"depth {depth}: records off differs"
    r.free()


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(M.scenes()))
def test_unordered_launches_take_identity_records(worldmap, name, size):
    """Below the order threshold the records are the identity; 1, 2, 3 and 5 lights (five_lights: more lights
    than shadow words)."""
    W, H = size
    text, t = M.scenes()[name]
    sc, r = _renderer(text, t, W, H)
    masked = name not in CHAIN_SCENES
    assert masked == (", reflection," in r.kernel_info()), r.kernel_info()
    for depth, kernel in ((10, "megakernel (specialised)"), (0, "primary-ray (specialised)")):
        got = _rows(r, 0, H, depth)
        _expect(r, kernel, records=masked, masks=masked)
        ref = _oracle_frame(name, W, H, depth)
        assert np.array_equal(got, ref), f"{name} depth {depth}: {int((got != ref).sum())} channels differ from the oracle"
    r.free()


def test_row_ranges_and_cyclic_bands(worldmap):
    import torch
    W, H = BIG
    text, t = M.scenes()["globes"]
    sc, r = _renderer(text, t, W, H)
    ref = _oracle_frame("globes", W, H, 10)
    # a geometry of >= RT_ORDER_MIN_TILES tiles calibrates on its first launch (the generic kernels at level 1:
    # no records) and is ordered from its second; a smaller one takes identity records at once
    def launches(n_rows):
        return 3 if ((W + 7) // 8) * ((n_rows + 7) // 8) >= 2048 else 1
    for y0, y1 in ((5, H - 3), (0, 9), (H - 13, H)):     # first rows no multiple of the tile; fewer rows than two tiles
        for launch in range(launches(y1 - y0)):
            part = _rows(r, y0, y1, 10)
            assert np.array_equal(part, ref[y0:y1]), f"rows [{y0}, {y1}), launch {launch} ({r.kernel_info()})"
        _expect(r, "megakernel (specialised)", records=True)
    assert launches(H - 8) == 3 and launches(9) == 1
    for label, y_first, band_rows, pitch, n_bands in M.geometries(H):
        for launch in range(launches(band_rows * n_bands)):
            out = torch.zeros((band_rows * n_bands, W, 4), dtype=torch.uint8, device="cuda")
            r.render_row_bands(y_first, band_rows, pitch, n_bands, out, max_depth=10)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            ys = M.frame_rows(H, y_first, band_rows, pitch, n_bands)
            keep = ys >= 0
            assert np.array_equal(got[keep], ref[ys[keep]]), f"{label}, launch {launch} ({r.kernel_info()})"
        _expect(r, "megakernel (specialised)", records=True)
    r.free()


def _moved_pair():
    a = M.scenes()["cubes_csg_3lights"][0]
    b = a.replace("cube(<-30, -15, 10>, 20, red)", "cube(<12, -15, -30>, 20, red)").replace(
        "set camera(<0, 10, -85>)", "set camera(<-25, 30, -70>)")
    assert a != b
    return a, b


def test_same_structure_upload_rebuilds_the_records(worldmap):
    """The stale-record hazard: scene b has scene a's structure, so the upload keeps the tile order and drops
    the masks -- records gathered from a's masks must never be found again."""
    import tinyraytracerinrust_amd as T
    W, H = BIG
    a, b = _moved_pair()
    sc, r = _renderer(a, 0.0, W, H)
    ref_a = _oracle_frame((a, 0.0), W, H, 10)
    for launch in range(3):                     # calibration (generic kernels at level 1), then ordered
        assert np.array_equal(_rows(r, 0, H, 10), ref_a), f"scene a, launch {launch} ({r.kernel_info()})"
    _expect(r, "megakernel (specialised)", records=True)
    r.upload(T.Scene.compile(b, 0.0, W, H, asset_dir=SCENES))
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    ref_b = _oracle_frame((b, 0.0), W, H, 10)
    assert not np.array_equal(ref_a, ref_b)
    for launch in ("first", "second"):
        got = _rows(r, 0, H, 10)
        _expect(r, "megakernel (specialised)", records=True)     # ordered at once: the order was kept
        assert np.array_equal(got, ref_b), f"scene b, {launch} launch after the upload: {int((got != ref_b).sum())} channels differ"
    r.free()


def test_two_streams_race_for_a_new_table(worldmap):
    """After an upload the first launch gathers the records on its stream; a launch queued at once on another
    stream, with no host synchronisation between them, must wait for that gather on the device."""
    import torch
    import tinyraytracerinrust_amd as T
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    # identity records of a launch too small to order, on a fresh context
    W, H = M.SIZES[1]
    text, t = M.scenes()["globes"]
    sc, r = _renderer(text, t, W, H)
    torch.cuda.synchronize()
    fa = r.render_rows(0, H, max_depth=10, stream=sa)
    fb = r.render_rows(0, H, max_depth=10, stream=sb)
    torch.cuda.synchronize()
    _expect(r, "megakernel (specialised)", records=True)
    ref = _oracle_frame("globes", W, H, 10)
    assert np.array_equal(fa.cpu().numpy(), ref) and np.array_equal(fb.cpu().numpy(), ref)
    r.free()
    # an order's records, rebuilt after a same-structure upload
    W, H = BIG
    a, b = _moved_pair()
    sc, r = _renderer(a, 0.0, W, H)
    for launch in range(2):
        _rows(r, 0, H, 10)
    r.upload(T.Scene.compile(b, 0.0, W, H, asset_dir=SCENES))
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    torch.cuda.synchronize()
    fa = r.render_rows(0, H, max_depth=10, stream=sa)
    fb = r.render_rows(0, H, max_depth=10, stream=sb)
    torch.cuda.synchronize()
    _expect(r, "megakernel (specialised)", records=True)
    ref = _oracle_frame((b, 0.0), W, H, 10)
    assert np.array_equal(fa.cpu().numpy(), ref) and np.array_equal(fb.cpu().numpy(), ref)
    r.free()


def test_f64_rows_bit_identical_with_records_without_and_generic(worldmap):
    """Level 2: the f64 launches run the specialised kernels (record prologue, scalar mask words); the same
    operations on the same values give the generic kernels' bits."""
    import tinyraytracerinrust_amd as T
    W, H = M.SIZES[0]
    text, t = M.scenes()["globes"]
    sc, r = _renderer(text, t, W, H, level=2)
    g = T.Renderer(0, specialize=0)
    g.set_kernel("mega")
    g.upload(sc)
    for depth, kernel in ((0, "primary-ray (specialised)"), (1, "megakernel (specialised)"), (2, "megakernel (specialised)"),
                          (10, "megakernel (specialised)")):
        r.set_tile_records(True)
        on = _rows(r, 0, H, depth, f64=True)
        _expect(r, kernel, records=True)
        r.set_tile_records(False)
        off = _rows(r, 0, H, depth, f64=True)
        _expect(r, kernel, records=False)
        assert on.tobytes() == off.tobytes(), f"depth {depth}: records on / off"
        gen = _rows(g, 0, H, depth, f64=True)
        assert g.kernel_variant() == "generic", g.kernel_info()
        assert on.tobytes() == gen.tobytes(), f"depth {depth}: specialised / generic"
    r.free()
    g.free()
