"""Traced tile masks (RT_OPT_TRACED_MASKS; rt_bodies.h trace_masks_body, k_masks.hip launch_records): a record
table's words narrowed, once per table, to what the entries' own pixels hit.  Dispatch only: every frame is
identical with the option 2, 0 and in the CPU oracle, and the words read back through rt_ctx_tile_records equal
what the oracle's rays say per tile: the prim word is the set of objects its primary rays hit
(orc_hit_signature); in an entry whose hits are all on the floor a shadow word holds a boxed bit exactly where a
pixel's light is occluded and the refl word is the set of objects the depth-1 rays hit (record_rays).  An entry
with a pixel on a boxed object keeps the predicate's shadow and refl words: the kernels read those under all ones
there (trace(): plane_tile is false), and the pass does not trace them.

Option 2, the megakernel pinned and masks forced: frames this small otherwise take neither."""
import re

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.test_gpu_lean_tiles import CAMERAS, FIVE_LIGHTS, REFRACTION, SCENE, SIZES, TWO_PLANES

pytestmark = pytest.mark.gpu

DEPTHS = (0, 1, 2, 10)
GLOBES_SIZE = (192, 108)                    # silhouette tiles and tiles inside the globe, a partial tile row
_truths = {}


def _text(camera):
    return SCENE.replace("<0, 10, -85>", CAMERAS[camera])


def _oracle(text, W, H, depth):
    from oracle import oracle as O
    return O.OracleScene(text, 0.0, W, H, max_depth=depth).render(0, H)[1]


def _truth(text, W, H):
    """Per pixel, from the oracle alone: the object the primary ray hits (-1: none), the bit set of occluded
    lights at that hit, and the object the depth-1 ray hits (-2: no such ray, -1: it misses).  Once per (scene, size)."""
    key = (text, W, H)
    if key not in _truths:
        import tinyraytracerinrust_amd as T
        from oracle import oracle as O
        orc = O.OracleScene(text, 0.0, W, H, max_depth=2)
        prim = np.full((H, W), -1, np.int64)
        occl = np.zeros((H, W), np.int64)
        refl = np.full((H, W), -2, np.int64)
        for y in range(H):
            for x in range(W):
                sig = orc.hit_signature(x, y)
                if sig < 0:
                    continue
                prim[y, x], occl[y, x] = sig % 4096 - 1, sig // 4096
                rec = orc.record_rays(x, y, cap=16)[0].view(T.RAY_RECORD_DTYPE)
                d1 = rec[rec["depth"] == 1]
                assert len(d1) <= 1                                        # reflection-only: a chain
                if len(d1):
                    refl[y, x] = d1[0]["object"] if d1[0]["intersected"] else -1
        _truths[key] = (prim, occl, refl, orc.n_lights)
    return _truths[key]


def _bits(objs):
    w = 0
    for o in np.unique(objs[objs >= 0]):
        w |= 1 << int(o)
    return w


def _upload(r, text, W, H):
    import tinyraytracerinrust_amd as T
    sc = T.Scene.compile(text, 0.0, W, H, asset_dir=SCENES)
    r.upload(sc)
    assert r.spec_wait(600_000) and r.kernel_variant() == "spec", r.kernel_info()
    return sc


def _new_renderer(level, traced=2):
    import tinyraytracerinrust_amd as T
    r = T.Renderer(0, specialize=level)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    r.set_traced_masks(traced)
    return r


@pytest.fixture(scope="module")
def renderer():
    """One context and (the camera is no part of a program's text) one program for the floor scene's tests, with the
    f64 kernels (level 2)."""
    r = _new_renderer(2)
    _upload(r, _text("front"), *SIZES[0])
    yield r
    r.free()


@pytest.fixture(scope="module")
def globes(worldmap):
    r = _new_renderer(1)
    _upload(r, scene_text("globes"), *GLOBES_SIZE)
    yield r
    r.free()


def _launch(r, shape, dtype, call):
    import torch
    out = torch.full(shape, 0xAB, dtype=torch.uint8, device="cuda")
    if dtype == "f64":
        out = out.view(torch.float64)
    call(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _counts(info):
    lean = re.search(r"; lean tiles: on \((\d+) entries\); sky fill: on \((\d+) render, (\d+) sky entries\)", info)
    assert lean, info
    return int(lean.group(1)), int(lean.group(3))


# ---------------------------------------------------------------- 1. frames
def _frames(r, text, W, H, depth, f64=True):
    ref = _oracle(text, W, H, depth)
    n_bands = (H + 23) // 24
    launches = {
        "rgba8": ((H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=depth, out=o)),
        "f64": ((H, W, 32), "f64", lambda o: r.render_rows(0, H, max_depth=depth, f64=True, out=o)),
        "rows 5..H-3": ((H - 8, W, 4), "u8", lambda o: r.render_rows(5, H - 3, max_depth=depth, out=o)),
        "bands 8 of 24": ((8 * n_bands, W, 4), "u8", lambda o: r.render_row_bands(0, 8, 24, n_bands, o, max_depth=depth)),
        "rgb8 bands": ((8 * n_bands, W, 3), "u8", lambda o: r.render_row_bands(0, 8, 24, n_bands, o, max_depth=depth)),
    }
    if not f64:                                                            # a level-1 program holds no f64 kernels
        del launches["f64"]
    got = {}
    for opt in (2, 0):
        r.set_traced_masks(opt)
        for name, (shape, dtype, call) in launches.items():
            got[opt, name] = _launch(r, shape, dtype, call)
            info = r.kernel_info()
            assert "tile masks: on" in info and "tile records: on" in info, info
            traced = opt == 2 and depth > 0                                # depth 0: the primary-ray kernel
            assert ("; traced masks: on; lean tiles: " if traced else "; traced masks: off; lean tiles: ") in info, (name, info)
    r.set_traced_masks(2)
    for name in launches:
        assert got[2, name].tobytes() == got[0, name].tobytes(), f"{name}: option 2 and 0 differ"
    assert np.array_equal(got[2, "rgba8"], ref)
    assert np.array_equal(got[2, "rows 5..H-3"], ref[5:H - 3])
    rows = np.arange(8 * n_bands)
    ys = (rows // 8) * 24 + rows % 8
    keep = ys < H
    assert np.array_equal(got[2, "bands 8 of 24"][keep], ref[ys[keep]])
    assert np.array_equal(got[2, "rgb8 bands"][keep], ref[ys[keep]][..., :3])
    assert (got[2, "bands 8 of 24"][~keep] == 0xAB).all() and (got[2, "rgb8 bands"][~keep] == 0xAB).all()
    if "f64" in launches:
        f64 = got[2, "f64"]
        assert np.array_equal(f64[..., 3], np.ones((H, W)))                # alpha: every pixel written, once
        assert np.array_equal((np.clip(f64[..., :3], 0.0, 1.0) * 255.0).astype(np.uint8), ref[..., :3])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_frames_identical_traced_untraced_and_oracle(renderer, camera, size, depth):
    W, H = size
    _upload(renderer, _text(camera), W, H)
    _frames(renderer, _text(camera), W, H, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_globes_frames_identical_traced_untraced_and_oracle(globes, depth):
    _frames(globes, scene_text("globes"), *GLOBES_SIZE, depth, f64=False)


# ---------------------------------------------------------------- 2. words against the oracle
def _check_words(r, sc, text, W, H):
    got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
    info = r.kernel_info()
    assert "; traced masks: on" in info and "megakernel (specialised)" in info, info
    recs = r.tile_records()
    pred_dev = r.tile_masks()
    pred, pinfo = sc.tile_masks()
    assert np.array_equal(pred_dev, pred)
    assert np.array_equal(got, _oracle(text, W, H, 2))
    prim, occl, refl, n_lights = _truth(text, W, H)
    plane_bit, boxed = 1 << pinfo["plane"], pinfo["boxed"]
    tx = (W + 7) // 8
    assert len(recs) == tx * ((H + 7) // 8)
    n_sky = n_lean = n_plane = n_narrowed = 0
    seen = set()
    for rec in recs:
        x0, r0, w = int(rec[0]) & 0x7fffffff, int(rec[1]), [int(v) for v in rec[2:]]
        says_lean = bool(int(rec[0]) >> 31)
        tile = (r0 // 8) * tx + x0 // 8
        seen.add(tile)
        p = [int(v) for v in pred[tile]]
        sl = (slice(r0, min(r0 + 8, H)), slice(x0, min(x0 + 8, W)))
        where = (tile, x0, r0, w, p)
        assert all(w[k] & ~p[k] == 0 for k in range(6)), where             # every traced word: a subset of the predicate's
        want_prim = _bits(prim[sl])
        assert w[0] == want_prim, where
        n_sky += want_prim == 0
        if want_prim != plane_bit:                                         # sky, or a pixel on a boxed object: prim alone
            assert w[1:] == p[1:] and not says_lean, where
            continue
        n_plane += 1
        any_occl = 0
        for l in range(n_lights):
            occluded = bool(((occl[sl] >> l) & 1).any())
            assert ((w[1 + l] & boxed) != 0) == occluded, (l, where)
            any_occl |= occluded
        assert w[1 + n_lights:5] == p[1 + n_lights:5], where
        want_refl = _bits(refl[sl])
        assert w[5] == want_refl, where
        lean = not any_occl and want_refl == 0
        assert says_lean == lean, where
        n_lean += lean
        n_narrowed += w != p
    assert seen == set(range(len(recs)))
    assert _counts(info) == (n_lean, n_sky), (info, n_lean, n_sky)
    return n_sky, n_lean, n_plane, n_narrowed


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_words_equal_the_oracle_rays(renderer, camera, size):
    W, H = size
    text = _text(camera)
    sc = _upload(renderer, text, W, H)
    n_sky, n_lean, n_plane, n_narrowed = _check_words(renderer, sc, text, W, H)
    print(f"{camera} {W}x{H}: {n_sky} sky, {n_lean} lean, {n_plane} floor-only entries, {n_narrowed} of them narrowed")
    if camera != "up":                                                     # (straight up: no floor to speak of)
        assert n_lean > 0


def test_globes_words_equal_the_oracle_rays(globes):
    W, H = GLOBES_SIZE
    text = scene_text("globes")
    sc = _upload(globes, text, W, H)
    n_sky, n_lean, n_plane, n_narrowed = _check_words(globes, sc, text, W, H)
    print(f"globes {W}x{H}: {n_sky} sky, {n_lean} lean, {n_plane} floor-only entries, {n_narrowed} of them narrowed")
    assert n_sky > 0 and n_lean > 0


# ---------------------------------------------------------------- 3. lifetime and scope
def test_same_structure_upload_with_the_camera_tilted_rebuilds_the_words(renderer):
    r = renderer
    W, H = SIZES[1]
    counts = []
    for camera in ("front", "tilted"):
        text = _text(camera)
        _upload(r, text, W, H)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        assert "; traced masks: on" in r.kernel_info(), r.kernel_info()
        counts.append(_counts(r.kernel_info()))
        assert np.array_equal(got, _oracle(text, W, H, 2)), camera
    assert counts[0] != counts[1] and min(counts[0][0], counts[1][0]) > 0, counts


@pytest.mark.parametrize("scene", ("two planes", "five lights", "refraction", "family"))
def test_scenes_outside_the_class_take_no_traced_table(scene):
    import tinyraytracerinrust_amd as T
    W, H = SIZES[1]
    r = _new_renderer(1)
    T.Scene.clear_families()
    try:
        if scene == "family":
            text = scene_text("spinning_globes")
            frames = [T.Scene.compile(text, f / 6, W, H, asset_dir=SCENES) for f in range(6)]
            T.Scene.register_family(frames)
            r.upload(frames[2])
            assert r.spec_wait(600_000) and "family of" in r.kernel_info(), r.kernel_info()
            from oracle import oracle as O
            ref = O.OracleScene(text, 2 / 6, W, H, max_depth=2).render(0, H)[1]
        else:
            text = {"two planes": TWO_PLANES, "refraction": REFRACTION, "five lights": FIVE_LIGHTS}[scene]
            _upload(r, text, W, H)
            ref = _oracle(text, W, H, 2)
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        info = r.kernel_info()
        assert "(specialised)" in info and "; traced masks: off; lean tiles: off" in info, info
        assert np.array_equal(got, ref), scene
    finally:
        T.Scene.clear_families()
        r.free()


def test_default_option_leaves_a_small_launch_untraced(renderer):
    r = renderer
    W, H = SIZES[0]
    text = _text("front")
    _upload(r, text, W, H)
    r.set_traced_masks(1)
    try:
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        info = r.kernel_info()
        assert "; traced masks: off; lean tiles: on (" in info and "tile records: on" in info, info
        assert np.array_equal(got, _oracle(text, W, H, 2))
    finally:
        r.set_traced_masks(2)


# ---------------------------------------------------------------- 4. the default's choice
def test_default_takes_a_traced_table_where_it_takes_the_masked_megakernel(worldmap):
    """The library's defaults (RT_OPT_TILE_MASKS 1, RT_OPT_TRACED_MASKS 1) on a frame large enough to calibrate (the
    size tests/test_gpu_tile_masks.py uses for the default's choice): the ordered launches take the masked or the
    mask-free megakernel by the calibration's verdict, and a traced table exactly with the former; exact either way.
    (Measured on an MI355X: 3600 tiles are fewer than the chip's 4096 wave slots, the launch is tail-bound, and the
    default says "tile masks: off; traced masks: off" here; the test below takes the default on the 4K frame, where
    the masks pay.)
    RT_OPT_TILE_MASKS 2 then forces the masked kernel on the same order: RT_OPT_TRACED_MASKS 1 stays off on a
    tail-bound order, 2 takes the table."""
    import tinyraytracerinrust_amd as T
    W, H = 640, 360
    text = scene_text("globes")
    r = T.Renderer(0, specialize=1)
    r.set_kernel("mega")
    try:
        r.upload(T.Scene.compile(text, 0.0, W, H, asset_dir=SCENES))
        assert r.spec_wait(600_000)
        ref = _oracle(text, W, H, 10)
        for launch in range(3):                     # calibration (generic), then ordered
            got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=10, out=o))
            assert np.array_equal(got, ref), r.kernel_info()
        info = r.kernel_info()
        print("default, 640x360 globes d10:", info.split("; traced masks")[1])
        assert "megakernel (specialised)" in info, info
        masked = "megakernel (specialised); tile masks: on; tile records: on" in info
        assert ("; traced masks: on" in info) == masked, info
        pays = masked
        r.set_tile_masks(2)                         # the masked megakernel on the same measured order
        for opt in (1, 2, 0):
            r.set_traced_masks(opt)
            got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=10, out=o))
            info = r.kernel_info()
            assert np.array_equal(got, ref), info
            assert "megakernel (specialised); tile masks: on; tile records: on" in info, info
            on = opt == 2 or (opt == 1 and pays)
            assert ("; traced masks: on" if on else "; traced masks: off") in info, (opt, info)
            if on:
                recs = r.tile_records()
                assert len(recs) >= (W // 8) * (H // 8) and _counts(info)[0] == int((recs[:, 0] >> 31).sum()), info
    finally:
        r.free()


def test_default_takes_the_traced_table_on_the_4k_frame_from_the_ninth_launch(worldmap):
    """Every option at the library's default on the headline frame (globes 3840x2160, depth 10), where the masks pay:
    launch 0 calibrates, launches 1..7 read the predicate's table (RT_TRACED_MIN_LAUNCHES: a fresh upload does not pay
    for the pass), launch 8 onwards the traced one.  The traced frame equals the RT_OPT_TRACED_MASKS 0 frame byte for
    byte (the frame tests/test_gpu_fullsize.py holds against the whole oracle frame) and the oracle on every 16th
    row; the counts are the oracle's bound (tools/mask_stats.py --truth, profiles/r24a_mask_truth.txt)."""
    import torch
    import tinyraytracerinrust_amd as T
    W, H, depth = 3840, 2160, 10
    text = scene_text("globes")
    r = T.Renderer(0, specialize=1)
    try:
        r.upload(T.Scene.compile(text, 0.0, W, H, asset_dir=SCENES))
        assert r.spec_wait(600_000)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        infos = []
        for launch in range(10):
            r.render_rows(0, H, max_depth=depth, out=out)
            torch.cuda.synchronize()
            infos.append(r.kernel_info())
        for launch in range(1, 8):
            assert "; traced masks: off; lean tiles: on (" in infos[launch], (launch, infos[launch])
            assert "megakernel (specialised); tile masks: on; tile records: on" in infos[launch], (launch, infos[launch])
        for launch in (8, 9):
            assert "; traced masks: on; lean tiles: on (" in infos[launch], (launch, infos[launch])
            assert "megakernel (specialised); tile masks: on; tile records: on" in infos[launch], (launch, infos[launch])
        assert _counts(infos[9]) == (57930, 46587), infos[9]               # lean, sky: the oracle's bound
        lean_pred, sky_pred = _counts(infos[7])
        assert lean_pred < 57930 and sky_pred < 46587, infos[7]
        recs = r.tile_records()
        assert len(recs) >= (W // 8) * (H // 8) and int((recs[:, 0] >> 31).sum()) == 57930 and int((recs[:, 2] == 0).sum()) == 46587
        traced = out.cpu().numpy()
        r.set_traced_masks(0)
        r.render_rows(0, H, max_depth=depth, out=out)
        torch.cuda.synchronize()
        assert "; traced masks: off" in r.kernel_info() and _counts(r.kernel_info()) == (lean_pred, sky_pred), r.kernel_info()
        assert traced.tobytes() == out.cpu().numpy().tobytes()
        from oracle import oracle as O
        ref = O.OracleScene(text, 0.0, W, H, max_depth=depth).render(0, H, row_step=16)[1]
        assert np.array_equal(traced[::16], ref)
        r.upload(T.Scene.compile(text, 0.0, W, H, asset_dir=SCENES))       # a new upload starts the count again
        assert r.spec_wait(600_000)
        r.set_traced_masks(1)
        r.render_rows(0, H, max_depth=depth, out=out)
        torch.cuda.synchronize()
        assert "; traced masks: off" in r.kernel_info() and "tile masks: on" in r.kernel_info(), r.kernel_info()
        assert traced.tobytes() == out.cpu().numpy().tobytes()
    finally:
        r.free()
