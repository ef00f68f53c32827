"""Sky tiles (RT_OPT_SKY_FILL; rt_device.h rows_entry, k_masks.hip tile_records_kernel): a wave of the masked
specialised kernels whose dispatch record holds an empty prim word stores BLACK and returns.  Culling and
dispatch only: every frame is identical with the option on, off and in the CPU oracle, in every output
format and launch geometry, and rt_ctx_kernel_info counts the entries that render and the ones that are sky."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(96, 72), (100, 75)]               # the second has a partial tile column and a partial tile row
# the floor and two boxed objects away from the origin the camera looks at, so that a camera under the origin
# looking up sees none of them
SCENE = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<45, -8, 10>, 12, red, 0.3))
draw(cube(<-45, -15, 20>, 18, blue, 0.2))
append light(<0, 30, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
CAMERAS = {"front": "<0, 10, -85>", "tilted": "<0, 45, -85>", "up": "<0, -24, -6>", "down": "<0, 60, -6>"}
TWO_PLANES = SCENE.replace("draw(sphere", "draw(plane(<0, 0, -1>, 120, rgb(0.3, 0.5, 0.3), 0.2))\ndraw(sphere", 1)


def _text(camera):
    return SCENE.replace("<0, 10, -85>", CAMERAS[camera])


def _oracle(text, W, H, depth):
    from oracle import oracle as O
    return O.OracleScene(text, 0.0, W, H, max_depth=depth).render(0, H)[1]


def _upload(r, text, W, H):
    import tinyraytracerinrust_amd as T
    r.upload(T.Scene.compile(text, 0.0, W, H))
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()


@pytest.fixture(scope="module")
def renderer():
    """One context and (the camera is no part of a program's text) one program for the module, with the f64
    kernels (level 2); the megakernel pinned and masks forced: frames this small otherwise take neither."""
    import tinyraytracerinrust_amd as T
    r = T.Renderer(0, specialize=2)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    _upload(r, _text("front"), *SIZES[0])
    yield r
    r.free()


def _counts(info):
    m = re.search(r"sky fill: on \((\d+) render, (\d+) sky entries\)", info)
    assert m, info
    return int(m.group(1)), int(m.group(2))


def _launch(r, shape, dtype, call):
    import torch
    out = torch.full(shape, 0xAB, dtype=torch.uint8, device="cuda")
    if dtype == "f64":
        out = out.view(torch.float64)
    call(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("depth", (0, 2))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_identical_on_off_and_oracle(renderer, size, depth):
    r = renderer
    W, H = size
    text = _text("front")
    _upload(r, text, W, H)
    ref = _oracle(text, W, H, depth)
    n_bands = (H + 23) // 24
    launches = {
        "rgba8": ((H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=depth, out=o)),
        "f64": ((H, W, 32), "f64", lambda o: r.render_rows(0, H, max_depth=depth, f64=True, out=o)),
        "rows 5..H-3": ((H - 8, W, 4), "u8", lambda o: r.render_rows(5, H - 3, max_depth=depth, out=o)),
        "bands 8 of 24": ((8 * n_bands, W, 4), "u8", lambda o: r.render_row_bands(0, 8, 24, n_bands, o, max_depth=depth)),
        "rgb8 bands": ((8 * n_bands, W, 3), "u8", lambda o: r.render_row_bands(0, 8, 24, n_bands, o, max_depth=depth)),
    }
    want = "primary-ray (specialised)" if depth == 0 else "megakernel (specialised)"
    got = {}
    for on in (True, False):
        r.set_sky_fill(on)
        for name, (shape, dtype, call) in launches.items():
            got[on, name] = _launch(r, shape, dtype, call)
            info = r.kernel_info()
            assert want in info and "tile masks: on" in info and "tile records: on" in info, info
            if on:
                n_render, n_sky = _counts(info)
                assert n_sky > 0 and n_render > 0, info
            else:
                assert "; sky fill: off; last launch:" in info, info
    r.set_sky_fill(True)
    for name in launches:
        assert got[True, name].tobytes() == got[False, name].tobytes(), f"{name}: on and off differ"
    assert np.array_equal(got[True, "rgba8"], ref)
    assert np.array_equal(got[True, "rows 5..H-3"], ref[5:H - 3])
    rows = np.arange(8 * n_bands)
    ys = (rows // 8) * 24 + rows % 8
    keep = ys < H
    assert np.array_equal(got[True, "bands 8 of 24"][keep], ref[ys[keep]])
    assert np.array_equal(got[True, "rgb8 bands"][keep], ref[ys[keep]][..., :3])
    assert (got[True, "bands 8 of 24"][~keep] == 0xAB).all() and (got[True, "rgb8 bands"][~keep] == 0xAB).all()
    f64 = got[True, "f64"]
    assert np.array_equal(f64[..., 3], np.ones((H, W)))                    # every pixel written, the sky's too
    sky = (ref[..., :3] == 0).all(axis=2)
    assert sky.any() and (f64[..., :3][sky] == 0.0).all()


def test_same_structure_upload_with_the_camera_tilted(renderer):
    """The tile order is kept across the upload, the masks and with them the sky set are not."""
    r = renderer
    W, H = SIZES[1]
    counts = []
    for camera in ("front", "tilted"):
        text = _text(camera)
        _upload(r, text, W, H)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        counts.append(_counts(r.kernel_info()))
        assert np.array_equal(got, _oracle(text, W, H, 2)), camera
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert all(a + b == tiles for a, b in counts) and counts[0] != counts[1], counts


@pytest.mark.parametrize("depth", (0, 2))
def test_camera_straight_up_and_straight_down(renderer, depth):
    r = renderer
    W, H = SIZES[1]
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    for camera, want in (("up", (0, tiles)), ("down", (tiles, 0))):
        text = _text(camera)
        _upload(r, text, W, H)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=depth, out=o))
        assert _counts(r.kernel_info()) == want, r.kernel_info()
        assert np.array_equal(got, _oracle(text, W, H, depth)), camera
        if camera == "up":
            assert (got[..., :3] == 0).all() and (got[..., 3] == 255).all()


def test_two_unbounded_planes_take_no_sky_fill():
    """A second plane keeps its bit in every prim word: the program holds no early-out and the info says off."""
    import tinyraytracerinrust_amd as T
    W, H = SIZES[1]
    r = T.Renderer(0, specialize=1)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    _upload(r, TWO_PLANES, W, H)
    for depth in (0, 2):
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=depth, out=o))
        info = r.kernel_info()
        assert "tile masks: on" in info and "; sky fill: off; last launch:" in info, info
        assert np.array_equal(got, _oracle(TWO_PLANES, W, H, depth)), depth
    r.free()
