"""Every instantiation the wavefront path's launches dispatch to by the scene's kind, the clamp form, the output
format and the fold span (k_wavefront.hip: wf_trace_kernel<REFR, FC>, wf_fold_kernel<SPAN, F64, FC>,
wf_fixup_kernel<REFR, F64, FC>; k_wf_pairs.hip: wfp_shade_kernel<REFR, FC>, both wfp_cand_kernel<SHADOW, true> -- the
forms for hierarchies too large for LDS are test_gpu_wavefront.py's large hierarchies) and the three branches of the
pixel store they share (f64, RGBA8, packed RGB8), at the smallest frame with a partial tile on both edges, 75 x 50: a
reflection-only scene and a ray tree, depths 1, 2 and 6 (fold spans 1, 2 and 3 + 3), RT_OPT_FAST_CLAMP on and off,
levels at the default capacity (the fold writes the pixels) and at 1 % (most come from the fix-up), the wave walk and
the pair path from level 0."""
import functools

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

W, H = 75, 50
TREE = ("draw(sphere(<0, 0, 0>, 30, red, 0.3, 0.6))\n"      # glass that also reflects, over a mirror floor
        "draw(plane(<0, 1, 0>, 35, blue, 0.5))")
TEXTS = {"globes": lambda: scene_text("globes"), "tree": lambda: TREE}
DEFAULT_CAP = 200


@functools.lru_cache(maxsize=None)
def _oracle(scene, d):
    from oracle import oracle as O
    rf, ru = O.OracleScene(TEXTS[scene](), 0.0, W, H, max_depth=d).render(0, H, f64=True)
    rf.setflags(write=False)
    ru.setflags(write=False)
    return rf, ru


def _renderer(scene, d):
    import tinyraytracerinrust_amd as T
    rt = T.RayTracer(W, H)
    rt.max_depth = d
    rt.load_scene(TEXTS[scene](), 0.0, asset_dir=SCENES)
    r = rt.renderer
    r.set_kernel("wavefront")
    return rt, r


@pytest.mark.parametrize("d", [1, 2, 6])
@pytest.mark.parametrize("scene", ["globes", "tree"])
def test_wavefront_every_instantiation(worldmap, scene, d):
    """One context per (scene, depth), the options switched on it: per setting the RGBA8 and f64 frames against
    the oracle, and the packed RGB8 frame (rt_render_row_bands_rgb8) equal to the RGBA8 frame's three channels."""
    import torch
    rf, ru = _oracle(scene, d)
    rt, r = _renderer(scene, d)
    for fc in (True, False):
        r.set_fast_clamp(fc)
        for cap in (DEFAULT_CAP, 1):
            r.set_wavefront_cap(cap)
            for pairs in (0, 2):
                r.set_wavefront_pairs(pairs)
                label = f"wavefront dispatch {scene} d={d} fc={fc} cap={cap} pairs={pairs}"
                gu, gf = r.render_rows_host(0, H), r.render_rows_host(0, H, f64=True)
                assert_close(gu, gf, ru, rf, label)
                rgb = torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device="cuda")
                r.render_row_bands(0, H, H, 1, rgb)
                torch.cuda.synchronize()
                assert np.array_equal(rgb.cpu().numpy(), gu[..., :3]), f"{label}: packed RGB8"


def test_wavefront_band_past_the_frame(worldmap):
    """Four bands of 8 rows from row 3 with pitch 16 at H = 50: the fourth starts at row 51.  The rows of lines
    that exist equal the oracle's; the eight output rows of the band past the frame are not written, by the fold
    (default capacity) or by the fix-up (1 %)."""
    import torch
    d = 6
    _, ru = _oracle("tree", d)
    rt, r = _renderer("tree", d)
    y_first, band_rows, pitch, n_bands = 3, 8, 16, 4
    lines = [y_first + b * pitch + k for b in range(n_bands) for k in range(band_rows)]
    inside = [i for i, y in enumerate(lines) if y < H]
    assert len(inside) == 24 and inside == list(range(24))
    for cap in (1, DEFAULT_CAP):
        r.set_wavefront_cap(cap)
        for pairs in (0, 2):
            r.set_wavefront_pairs(pairs)
            out = torch.full((n_bands * band_rows, W, 4), 0xA5, dtype=torch.uint8, device="cuda")
            r.render_row_bands(y_first, band_rows, pitch, n_bands, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[:24], ru[[lines[i] for i in inside]]), f"band rows, cap={cap} pairs={pairs}"
            assert (got[24:] == 0xA5).all(), f"rows of the band past the frame were written, cap={cap} pairs={pairs}"
