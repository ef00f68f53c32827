"""Lean tiles (RT_OPT_LEAN_TILES; rt_bodies.h lean_body / lean_check_body, k_masks.hip launch_records): the entries
of a megakernel launch whose rays can meet the floor alone are rendered by the program's lean kernel, launched
ahead of the megakernel, whose waves of those entries return at once.  Dispatch only: every frame is identical
with the option on, off and in the CPU oracle, in every output format and launch geometry, and the count
rt_ctx_kernel_info gives equals one made on the CPU: the candidate tiles of the host's mask predicate
(rt_scene_tile_masks) minus the tiles in which the oracle's ray records show a depth-1 ray of some pixel
hitting anything.

That subtraction was empty everywhere it was looked for.  With the oracle alone, over the family the check
exists for -- the camera 1e-3 ... 1 above the floor looking horizontally (LOW below: 25 heights spaced evenly
in the logarithm and 8 round ones, at both sizes) -- no candidate tile holds a pixel whose reflected ray hits:
0 demoted of 34 candidates at 96x72 and of 47 at 100x75 at every height.  No hook forces the case; the equality
below would catch a demotion the day a scene has one."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(96, 72), (100, 75)]               # the second has a partial tile column and a partial tile row
# a floor, two boxed objects off-centre and two lights (the scene's own and the appended one)
SCENE = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<45, -8, 10>, 12, red, 0.3))
draw(cube(<-45, -15, 20>, 18, blue, 0.2))
append light(<0, 30, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
CAMERAS = {"front": "<0, 10, -85>", "tilted": "<0, 45, -85>", "up": "<0, -24, -6>", "down": "<0, 60, -6>"}
# the camera looks at the origin: horizontally, %r above the floor
LOW = """
draw(plane(<0, 1, 0>, %r, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<45, 13, 10>, 12, red, 0.3))
draw(cube(<-45, 10, 20>, 18, blue, 0.2))
append light(<0, 30, -35>, white * 0.5, 100)
set camera(<0, 0, -85>)
"""
TWO_PLANES = SCENE.replace("draw(sphere", "draw(plane(<0, 0, -1>, 120, rgb(0.3, 0.5, 0.3), 0.2))\ndraw(sphere", 1)
REFRACTION = SCENE.replace("red, 0.3", "red, 0.0, 0.8")
FIVE_LIGHTS = SCENE + "".join(f"append light(<{x}, 30, -35>, white * 0.2, 100)\n" for x in (-40, -20, 20))
_cpu_counts = {}


def _text(camera):
    return SCENE.replace("<0, 10, -85>", CAMERAS[camera])


def _oracle(text, W, H, depth):
    from oracle import oracle as O
    return O.OracleScene(text, 0.0, W, H, max_depth=depth).render(0, H)[1]


def _cpu_lean(text, W, H):
    """(lean entries, candidates) of the whole frame, on the CPU: the host predicate's candidate tiles minus the
    tiles where the oracle records a depth-1 ray that hits.  Computed once per (scene, size)."""
    key = (text, W, H)
    if key in _cpu_counts:
        return _cpu_counts[key]
    import tinyraytracerinrust_amd as T
    from oracle import oracle as O
    s = T.Scene.compile(text, 0.0, W, H)
    words, info = s.tile_masks()
    orc = O.OracleScene(text, 0.0, W, H, max_depth=2)
    keep = np.uint32(~(1 << info["plane"]) & 0xffffffff)
    cand = (words[:, 0] != 0) & ((words[:, 0] & keep) == 0) & ((words[:, 5] & keep) == 0)
    for l in range(orc.n_lights):
        cand &= (words[:, 1 + l] & keep) == 0
    tx = (W + 7) // 8
    demoted = 0
    for t in np.flatnonzero(cand):
        x0, y0 = (t % tx) * 8, (t // tx) * 8
        hit = False
        for y in range(y0, min(y0 + 8, H)):
            for x in range(x0, min(x0 + 8, W)):
                r = orc.record_rays(x, y, cap=16)[0].view(T.RAY_RECORD_DTYPE)
                hit = hit or bool(((r["depth"] == 1) & (r["intersected"] != 0)).any())
        demoted += hit
    _cpu_counts[key] = (int(cand.sum()) - demoted, int(cand.sum()))
    return _cpu_counts[key]


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


def _lean(info):
    m = re.search(r"; lean tiles: on \((\d+) entries\); sky fill: ", info)
    assert m, info
    return int(m.group(1))


def _sky(info):
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
    tiles = {name: ((W + 7) // 8) * ((shape[0] + 7) // 8) for name, (shape, _, _) in launches.items()}
    got = {}
    for on in (True, False):
        r.set_lean_tiles(on)
        for name, (shape, dtype, call) in launches.items():
            got[on, name] = _launch(r, shape, dtype, call)
            info = r.kernel_info()
            assert "tile masks: on" in info and "tile records: on" in info, info
            n_render, n_sky = _sky(info)
            assert n_render + n_sky == tiles[name], (name, info)           # render counts every non-sky entry, as before
            if on and depth > 0:
                assert "megakernel (specialised)" in info, info
                assert 0 < _lean(info) <= n_render, (name, info)
            else:                                                          # the option, or the primary-ray kernel
                assert "; lean tiles: off; sky fill: on" in info, info
    r.set_lean_tiles(True)
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
    assert np.array_equal(f64[..., 3], np.ones((H, W)))                    # alpha: every pixel written, once
    assert np.array_equal((np.clip(f64[..., :3], 0.0, 1.0) * 255.0).astype(np.uint8), ref[..., :3])
    if depth > 0:
        assert _cpu_lean(text, W, H)[0] > 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", ("front", "tilted", "down"))
def test_lean_count_equals_the_cpu_count(renderer, scene, size):
    r = renderer
    W, H = size
    text = _text(scene)
    _upload(r, text, W, H)
    got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
    want, cand = _cpu_lean(text, W, H)
    assert cand > 0 and _lean(r.kernel_info()) == want, (r.kernel_info(), want, cand)
    assert np.array_equal(got, _oracle(text, W, H, 2)), scene


def test_low_horizontal_camera_count_equals_the_cpu_count():
    """One member of the family the docstring's search covered (its own program: the floor's height is in the
    text; level 1, one compile for both sizes)."""
    import tinyraytracerinrust_amd as T
    r = T.Renderer(0, specialize=1)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    text = LOW % 0.01
    try:
        for W, H in SIZES:
            _upload(r, text, W, H)
            got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
            want, cand = _cpu_lean(text, W, H)
            assert cand > 0 and _lean(r.kernel_info()) == want, (r.kernel_info(), want, cand)
            assert np.array_equal(got, _oracle(text, W, H, 2)), (W, H)
    finally:
        r.free()


def test_same_structure_upload_with_the_camera_tilted(renderer):
    """The tile order is kept across the upload; the masks, and with them the lean set, are not."""
    r = renderer
    W, H = SIZES[1]
    counts = []
    for camera in ("front", "tilted"):
        text = _text(camera)
        _upload(r, text, W, H)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        counts.append(_lean(r.kernel_info()))
        assert np.array_equal(got, _oracle(text, W, H, 2)), camera
    assert counts[0] != counts[1] and min(counts) > 0, counts


def test_camera_straight_up_and_straight_down(renderer):
    r = renderer
    W, H = SIZES[1]
    for camera in ("up", "down"):
        text = _text(camera)
        _upload(r, text, W, H)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        want = 0 if camera == "up" else _cpu_lean(text, W, H)[0]           # bare floor below, nothing above
        assert _lean(r.kernel_info()) == want and (camera == "up" or want > 0), r.kernel_info()
        assert np.array_equal(got, _oracle(text, W, H, 2)), camera


@pytest.mark.parametrize("scene", ("two planes", "refraction", "five lights"))
def test_scenes_outside_the_class_take_no_lean_kernel(scene):
    """A second unbounded object, a transparent object, a fifth light: the program holds no lean kernel."""
    import tinyraytracerinrust_amd as T
    text = {"two planes": TWO_PLANES, "refraction": REFRACTION, "five lights": FIVE_LIGHTS}[scene]
    W, H = SIZES[1]
    assert T.Scene.compile(text, 0.0, W, H).lean_report() == ""
    r = T.Renderer(0, specialize=1)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    try:
        _upload(r, text, W, H)
        for depth in (0, 2):
            got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=depth, out=o))
            info = r.kernel_info()
            assert "(specialised)" in info and "; lean tiles: off; sky fill: " in info, info
            assert np.array_equal(got, _oracle(text, W, H, depth)), (scene, depth)
    finally:
        r.free()


def test_lean_kernel_resources():
    """The lean kernel's line of rt_scene_lean_report: 8 waves per SIMD, nothing spilled, no scratch."""
    import tinyraytracerinrust_amd as T
    lines = {}
    for line in T.Scene.compile(SCENE, 0.0, *SIZES[0]).lean_report().splitlines():
        name, rest = line.split(": ", 1)
        f = rest.split()
        lines[name] = {f[i]: f[i + 1] for i in range(0, len(f) - 1, 2)}
    assert set(lines) == {"rt_spec_lean_0", "rt_spec_lean_check"}, lines
    k = lines["rt_spec_lean_0"]
    assert int(k["occupancy"]) == 8 and int(k["spilled"]) == 0 and int(k["scratch"]) == 0, k
