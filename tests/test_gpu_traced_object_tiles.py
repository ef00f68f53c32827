"""Traced tile masks on object tiles (RT_OPT_TRACED_MASKS 3, and the table the default takes; rt_bodies.h
trace_masks_body `objects`): an entry with a pixel on a boxed object is traced too -- every lane that hit anything,
its shadow words from all boxed objects of the scene, its refl word under all ones -- and its record's r0 carries
the sign bit, on which trace() reads words 1..5 for every depth-0 hit of the entry.  Dispatch only: every frame is
identical under the values 3, 2 and 0 and in the CPU oracle, and every flagged entry's words equal what the oracle's
rays say for its pixels: light l's word holds a boxed bit exactly where some pixel has light l occluded
(orc_hit_signature), the refl word is the set of objects the depth-1 rays hit (record_rays).  Value 2 keeps the
floor-only form (tests/test_gpu_traced_masks.py): no flag, object entries with the predicate's words.

Megakernel pinned and masks forced: frames this small otherwise take neither."""
import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.test_gpu_lean_tiles import CAMERAS, FIVE_LIGHTS, REFRACTION, SIZES, TWO_PLANES
from tests.test_gpu_traced_masks import DEPTHS, GLOBES_SIZE, _bits, _counts, _launch, _oracle, _text, _truth, _upload

pytestmark = pytest.mark.gpu

FLAG = 0x80000000
# The hazard and the mixed entries, one program.  The red sphere floats below the horizon under a light straight
# above it: its lower side is self-shadowed, while the floor the same tiles' cones meet lies far behind the shadow
# of its box, so the predicate's shadow word there holds no boxed bit.  The blue sphere covers the frame's
# bottom-right corner (at 100x75 the entry cut by both edges); the green one crosses the horizon (entries with
# object, floor and sky lanes at once).
HAZARD = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<-10, -5, 0>, 12, red, 0.3))
draw(sphere(<24, -10, -50>, 8, blue, 0.2))
draw(sphere(<45, 24, 30>, 14, green, 0.4))
append light(<-10, 90, 0>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""


def _new_renderer(level):
    import tinyraytracerinrust_amd as T
    r = T.Renderer(0, specialize=level)
    r.set_kernel("mega")
    r.set_tile_masks(2)
    r.set_traced_masks(3)
    return r


@pytest.fixture(scope="module")
def renderer():
    r = _new_renderer(2)                                                   # the f64 kernels too
    _upload(r, _text("front"), *SIZES[0])
    yield r
    r.free()


@pytest.fixture(scope="module")
def globes(worldmap):
    r = _new_renderer(1)
    _upload(r, scene_text("globes"), *GLOBES_SIZE)
    yield r
    r.free()


@pytest.fixture(scope="module")
def hazard():
    r = _new_renderer(1)
    _upload(r, HAZARD, *SIZES[1])
    yield r
    r.free()


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
    try:
        for opt in (3, 2, 0):
            r.set_traced_masks(opt)
            for name, (shape, dtype, call) in launches.items():
                got[opt, name] = _launch(r, shape, dtype, call)            # over 0xAB
                info = r.kernel_info()
                assert "tile masks: on" in info and "tile records: on" in info, info
                traced = opt != 0 and depth > 0                            # depth 0: the primary-ray kernel
                assert ("; traced masks: on; lean tiles: " if traced else "; traced masks: off; lean tiles: ") in info, (name, info)
                if name == "rgba8" and opt != 3:                           # only value 3's table carries the flag
                    assert not (r.tile_records()[:, 1] >> 31).any(), (opt, info)
    finally:
        r.set_traced_masks(3)
    for name in launches:
        assert got[3, name].tobytes() == got[2, name].tobytes(), f"{name}: values 3 and 2 differ"
        assert got[3, name].tobytes() == got[0, name].tobytes(), f"{name}: values 3 and 0 differ"
    assert np.array_equal(got[3, "rgba8"], ref)
    assert np.array_equal(got[3, "rows 5..H-3"], ref[5:H - 3])
    rows = np.arange(8 * n_bands)
    ys = (rows // 8) * 24 + rows % 8
    keep = ys < H
    assert np.array_equal(got[3, "bands 8 of 24"][keep], ref[ys[keep]])
    assert np.array_equal(got[3, "rgb8 bands"][keep], ref[ys[keep]][..., :3])
    assert (got[3, "bands 8 of 24"][~keep] == 0xAB).all() and (got[3, "rgb8 bands"][~keep] == 0xAB).all()
    if "f64" in launches:
        f = got[3, "f64"]
        assert np.array_equal(f[..., 3], np.ones((H, W)))                  # alpha: every pixel written, once
        assert np.array_equal((np.clip(f[..., :3], 0.0, 1.0) * 255.0).astype(np.uint8), ref[..., :3])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_frames_identical_under_3_2_0_and_oracle(renderer, camera, size, depth):
    W, H = size
    _upload(renderer, _text(camera), W, H)
    _frames(renderer, _text(camera), W, H, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_globes_frames_identical_under_3_2_0_and_oracle(globes, depth):
    _frames(globes, scene_text("globes"), *GLOBES_SIZE, depth, f64=False)


@pytest.mark.parametrize("depth", DEPTHS)
def test_hazard_frames_identical_under_3_2_0_and_oracle(hazard, depth):
    _frames(hazard, HAZARD, *SIZES[1], depth, f64=False)


# ---------------------------------------------------------------- 2. words against the oracle's rays, the flag
def _records(r, W, H, opt):
    r.set_traced_masks(opt)
    try:
        got = _launch(r, (H, W, 4), "u8", lambda o: r.render_rows(0, H, max_depth=2, out=o))
        info = r.kernel_info()
        assert "; traced masks: on" in info and "megakernel (specialised)" in info, info
        return got, r.tile_records(), _counts(info)
    finally:
        r.set_traced_masks(3)


def _check_words(r, sc, text, W, H):
    """Every entry of the value-3 table against the oracle's rays and the value-2 table; returns what it met."""
    got, recs, counts = _records(r, W, H, 3)
    got2, recs2, counts2 = _records(r, W, H, 2)
    assert np.array_equal(got, _oracle(text, W, H, 2)) and got.tobytes() == got2.tobytes()
    pred, pinfo = sc.tile_masks()
    prim, occl, refl, n_lights = _truth(text, W, H)
    plane, boxed = pinfo["plane"], pinfo["boxed"]
    tx = (W + 7) // 8
    assert len(recs) == len(recs2) == tx * ((H + 7) // 8)
    assert not (recs2[:, 1] & FLAG).any()                                  # value 2: no entry is flagged
    # prim words, lean bits (x0), positions and the sky and lean counts: value 2's
    assert np.array_equal(recs[:, 0], recs2[:, 0]) and np.array_equal(recs[:, 1] & ~np.uint32(FLAG), recs2[:, 1])
    assert np.array_equal(recs[:, 2], recs2[:, 2]) and counts == counts2, (counts, counts2)
    met = {"flagged": 0, "hazard": 0, "no ray": 0, "mixed": 0, "edges": 0, "inside": 0}
    for rec, rec2 in zip(recs, recs2):
        x0, r0, w = int(rec[0]) & 0x7fffffff, int(rec[1]) & 0x7fffffff, [int(v) for v in rec[2:]]
        flagged = bool(int(rec[1]) & FLAG)
        tile = (r0 // 8) * tx + x0 // 8
        p = [int(v) for v in pred[tile]]
        sl = (slice(r0, min(r0 + 8, H)), slice(x0, min(x0 + 8, W)))
        where = (tile, x0, r0, w, p)
        on_object = (prim[sl] >= 0) & (prim[sl] != plane)
        assert flagged == bool(on_object.any()), where                     # every entry with a valid pixel on a boxed object
        if not flagged:
            assert w == [int(v) for v in rec2[2:]], where                  # floor-only and sky entries: value 2's words
            continue
        assert not int(rec[0]) >> 31 and w[0] == _bits(prim[sl]) and w[0] != 0, where
        met["flagged"] += 1
        hit = prim[sl] >= 0
        for l in range(n_lights):
            occluded = bool((((occl[sl] >> l) & 1) != 0)[hit].any())
            assert ((w[1 + l] & boxed) != 0) == occluded, (l, where)
            met["hazard"] += (w[1 + l] & ~p[1 + l] & boxed) != 0           # a boxed bit the predicate's word lacks
        assert w[5] == _bits(refl[sl]), where
        met["no ray"] += bool((refl[sl] == -2).all())
        if (refl[sl] == -2).all():
            assert w[5] == 0, where
        met["mixed"] += bool((prim[sl] == plane).any() and (prim[sl] < 0).any())
        met["edges"] += x0 + 8 > W and r0 + 8 > H
        met["inside"] += bool(on_object.all() and on_object.size == 64)
    return met


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", ("front", "tilted"))                    # (up and down: no object in view)
def test_words_equal_the_oracle_rays(renderer, camera, size):
    W, H = size
    text = _text(camera)
    sc = _upload(renderer, text, W, H)
    met = _check_words(renderer, sc, text, W, H)
    print(f"{camera} {W}x{H}: {met}")
    assert met["flagged"] > 0


def test_globes_words_equal_the_oracle_rays(globes):
    W, H = GLOBES_SIZE
    text = scene_text("globes")
    sc = _upload(globes, text, W, H)
    met = _check_words(globes, sc, text, W, H)
    print(f"globes {W}x{H}: {met}")
    # silhouette entries, entries wholly inside an object, and entries whose pixels spawn no ray (the globe reflects nothing)
    assert met["flagged"] > met["inside"] > 0 and met["no ray"] > 0


def _hazard_on_cpu(W, H):
    """The hazard, from the host's predicate and the oracle alone: tiles with an object pixel whose light l is
    occluded while the predicate's shadow[l] word holds no boxed bit; and the mixed and the edge-cut object tiles."""
    import tinyraytracerinrust_amd as T
    sc = T.Scene.compile(HAZARD, 0.0, W, H)
    pred, pinfo = sc.tile_masks()
    prim, occl, refl, n_lights = _truth(HAZARD, W, H)
    plane, boxed = pinfo["plane"], pinfo["boxed"]
    tx = (W + 7) // 8
    self_shadow = mixed = edges = 0
    for tile in range(len(pred)):
        x0, r0 = (tile % tx) * 8, (tile // tx) * 8
        sl = (slice(r0, min(r0 + 8, H)), slice(x0, min(x0 + 8, W)))
        if not ((prim[sl] >= 0) & (prim[sl] != plane)).any():
            continue
        for l in range(n_lights):
            self_shadow += bool(((occl[sl] >> l) & 1).any()) and (int(pred[tile][1 + l]) & boxed) == 0
        mixed += bool((prim[sl] == plane).any() and (prim[sl] < 0).any())
        edges += x0 + 8 > W and r0 + 8 > H
    return self_shadow, mixed, edges


def test_hazard_self_shadow_mixed_and_edge_entries(hazard):
    W, H = SIZES[1]
    self_shadow, mixed, edges = _hazard_on_cpu(W, H)                       # the scene has the cases, before the GPU says so
    assert self_shadow > 0 and mixed > 0 and edges == 1, (self_shadow, mixed, edges)
    sc = _upload(hazard, HAZARD, W, H)
    met = _check_words(hazard, sc, HAZARD, W, H)
    print(f"hazard {W}x{H}: {met}; on the CPU: {self_shadow} self-shadowed, {mixed} mixed, {edges} edge-cut")
    assert met["hazard"] >= self_shadow and met["mixed"] == mixed and met["edges"] == edges, met


# ---------------------------------------------------------------- 3. lifetime and scope
def test_same_structure_upload_with_the_camera_tilted_rebuilds_the_words(renderer):
    r = renderer
    W, H = SIZES[1]
    tables = []
    for camera in ("front", "tilted"):
        text = _text(camera)
        _upload(r, text, W, H)
        got, recs, counts = _records(r, W, H, 3)
        assert np.array_equal(got, _oracle(text, W, H, 2)), camera
        assert (recs[:, 1] & FLAG).any()
        tables.append(recs)
    assert not np.array_equal(tables[0], tables[1])


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


def test_option_setter_rejects_values_outside_0_to_3(renderer):
    try:
        for bad in (-1, 4):
            with pytest.raises(Exception):
                renderer.set_traced_masks(bad)
        for ok in (0, 1, 2, 3):
            renderer.set_traced_masks(ok)
    finally:
        renderer.set_traced_masks(3)
