"""The tighter tile-mask predicate (csrc/rt_tilemask.h: vertex sets of the required leaves, the sphere bound,
the clip at the plane through the light) on the CPU, through rt_scene_tile_masks.  Soundness by
test_tile_masks_host.py's method: no object the oracle's rays hit may have its bit clear (primary hits, and the
occluder of every floor pixel in shadow, orc_hit_signature per pixel); the masks do get tighter than the
world boxes alone can make them; and degenerate inputs never clear a bit by accident."""
import math

import numpy as np
import pytest

from tests import tile_mask_scenes as M
from tests import tile_mask_tight_scenes as X
from tests.conftest import SCENES

ONES = 0xFFFFFFFF
PRIM, SHADOW, REFL = 0, 1, 5


def _check_sound(sc, sig, W, H, name):
    tiles_x = (W + 7) // 8
    n_prim = n_shadow = 0
    for label, y_first, band_rows, pitch, n_bands in M.geometries(H):
        words, info = sc.tile_masks(y_first, band_rows, pitch, n_bands)
        assert info["valid"]
        n = sc.info()["objects"]
        only_plane = [o for o in range(n) if not (info["boxed"] >> o) & 1] == [info["plane"]]
        ys = M.frame_rows(H, y_first, band_rows, pitch, n_bands)
        for r, y in enumerate(ys):
            if y < 0:
                continue
            for x in range(W):
                s = int(sig[y, x])
                if s < 0:
                    continue
                w = words[(r // 8) * tiles_x + x // 8]
                obj, occl = (s & 4095) - 1, s >> 12
                assert (int(w[PRIM]) >> obj) & 1, f"{name} {label} pixel ({x}, {y}): hit object {obj}, prim {int(w[PRIM]):#x}"
                n_prim += 1
                if obj != info["plane"]:
                    continue
                for l in range(4):
                    if (occl >> l) & 1:
                        sw = int(w[SHADOW + l])
                        assert sw != 0 and (not only_plane or sw & info["boxed"]), \
                            f"{name} {label} pixel ({x}, {y}): light {l} occluded, shadow word {sw:#x}"
                        n_shadow += 1
    return n_prim, n_shadow


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(X.scenes()))
def test_one_object_scenes_keep_the_occluder(name, size):
    import tinyraytracerinrust_amd as T
    W, H = size
    sc = T.Scene.compile(X.scenes()[name], 0.0, W, H)
    words, info = sc.tile_masks()
    assert info["plane"] == 0 and info["boxed"] == 2, info            # the floor, and one boxed object
    n_prim, n_shadow = _check_sound(sc, X.signatures(name, W, H), W, H, name)
    assert n_prim > 0 and n_shadow > 0, (n_prim, n_shadow)             # the object does cast a shadow in view
    print(f"{name} {W}x{H}: {n_prim} primary hits, {n_shadow} occluded floor shadow rays checked")


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["globes", "three_cubes", "ground_star"])
def test_whole_scenes_keep_every_object_the_oracle_hits(name, size):
    import tinyraytracerinrust_amd as T
    W, H = size
    text, t = M.scenes()[name]
    sc = T.Scene.compile(text, t, W, H, asset_dir=SCENES)
    n_prim, _ = _check_sound(sc, M.signatures(name, W, H), W, H, name)
    assert n_prim > 0


def test_globes_masks_are_tighter_than_the_world_boxes_allow():
    """globes.scene 96x72 against the predicate with the world boxes alone, computed here from the scene's boxes
    (tile_mask_tight_scenes.world_box_walks).  Objects 3 (claw), 4 (globe) and 5 (axis rod, 2 x 40 x 2 in a
    56 x 50 x 18 world box) rise above light 1 at (0, 0, -35), so their world boxes cross every side plane of every
    floor tile's shadow pyramid beyond the apex.  No word may hold a boxed bit the world boxes rule out (the
    world box is still asked first); the boxed bits per walk must be fewer; each of the three objects must leave
    shadow[1] in some floor tiles where its world box keeps it; and the rod, whose box is the loosest, must
    fall to under half of its world box's count in shadow[1] and in prim."""
    import tinyraytracerinrust_amd as T
    text, t = M.scenes()["globes"]
    sc = T.Scene.compile(text, t, 96, 72, asset_dir=SCENES)
    words, info = sc.tile_masks()
    boxed = info["boxed"]
    ref = X.world_box_walks(sc, 96, 72)
    assert len(ref) == len(words)
    bits_of = lambda w: {o for o in range(32) if (int(w) & boxed) >> o & 1}
    got_bits = ref_bits = walks = 0
    count = {"got": {o: 0 for o in (3, 4, 5)}, "ref": {o: 0 for o in (3, 4, 5)}}
    rod_prim = {"got": 0, "ref": 0}
    n_floor = 0
    for w, (prim, shadow, refl) in zip(words, ref):
        assert (shadow is None) == (int(w[SHADOW]) == ONES)              # the same floor tiles
        pairs = [(w[PRIM], prim)]
        if shadow is not None:
            n_floor += 1
            pairs += [(w[SHADOW + l], s) for l, s in enumerate(shadow)] + [(w[REFL], refl)]
            for o in (3, 4, 5):
                count["got"][o] += (int(w[SHADOW + 1]) >> o) & 1
                count["ref"][o] += o in shadow[1]
        rod_prim["got"] += (int(w[PRIM]) >> 5) & 1
        rod_prim["ref"] += 5 in prim
        for word, allowed in pairs:
            assert bits_of(word) <= allowed, (bits_of(word), allowed)
            got_bits += len(bits_of(word))
            ref_bits += len(allowed)
            walks += 1
    print(f"globes 96x72: {walks} walks, {n_floor} floor tiles; boxed bits per walk {got_bits / walks:.3f}, world boxes alone "
          f"{ref_bits / walks:.3f}; shadow[1] tiles per object {count}; rod in prim {rod_prim}")
    assert n_floor > 20 and got_bits < ref_bits
    for o in (3, 4, 5):
        assert count["got"][o] < count["ref"][o], (o, count)
    assert 2 * count["got"][5] < count["ref"][5] and 2 * rod_prim["got"] < rod_prim["ref"], (count, rod_prim)


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rod_shadow_bit_is_confined_to_a_band_of_tile_columns(size):
    """The light lower than the rod's top (light 1 of the first group): the rod's world box crosses the
    plane through the light, and unclipped its bit would fill whole tile rows."""
    import tinyraytracerinrust_amd as T
    W, H = size
    sc = T.Scene.compile(X.scenes()["rod-low_above_beside"], 0.0, W, H)
    words, info = sc.tile_masks()
    tiles_x = (W + 7) // 8
    grid = words.reshape(-1, tiles_x, 6)
    floor = grid[:, :, SHADOW + 1] != ONES
    bit = ((grid[:, :, SHADOW + 1] >> 1) & 1).astype(bool) & floor
    assert bit.any()
    cols = np.flatnonzero(bit.any(axis=0))
    print(f"rod {W}x{H}: shadow[1] bit in tile columns {cols.min()}..{cols.max()} of {tiles_x}")
    assert cols.max() - cols.min() + 1 <= tiles_x // 2
    for row in range(grid.shape[0]):                                   # and within a row, never the whole row
        if floor[row].all():
            assert not bit[row].all(), row


def _programmatic(W, H, build):
    import tinyraytracerinrust_amd as T
    rt = T.RayTracer(W, H)
    rt.add_object(rt.plane((0, 1, 0), 25.01), T.solid_material((0.6, 0.6, 0.6, 1.0), 0.3))
    build(T, rt)
    rt.set_camera_from_vector((0, 10, -85))
    return rt.scene


def _bounds(sc):
    """rt_scene_describe's lines on the tile masks' bounds: object -> (vertex sets, has a ball)"""
    import re
    return {int(m.group(1)): (int(m.group(2)), bool(int(m.group(3))))
            for m in re.finditer(r"tile-mask bounds object (\d+): sets (\d+) ball (\d+)", sc.describe())}


def test_which_objects_take_which_bounds():
    """A sphere takes its leaf's set and a ball; the difference shell likewise (only the outer sphere is
    required); the rod one set per leaf and no ball (its sphere is scaled (1, 100, 1)); the ellipsoid, a sphere
    under a non-similarity, a set and NO ball; the column drops the set of its far-reaching leaf."""
    import tinyraytracerinrust_amd as T
    want = {"sphere": (1, True), "shell": (1, True), "bitten": (1, True), "rod": (2, False), "slab": (1, False),
            "ellipsoid": (1, False), "column": (1, False)}
    for obj, w in want.items():
        sc = T.Scene.compile(X.scenes()[obj + "-top_face"], 0.0, 96, 72)
        assert _bounds(sc) == {1: w}, (obj, _bounds(sc))


def test_a_dropped_set_leaves_the_other_bounds():
    """CSG objects whose world box stays finite through the cube while the sphere leaf's own set must go: a
    singular sphere transform (no inverse), and a sphere whose box reaches beyond RT_CULL_COORD_MAX (the column
    of tile_mask_tight_scenes, whose soundness the oracle test above checks).  With the singular leaf the
    object keeps exactly the cube's bounds: its words equal the plain cube's."""
    import tinyraytracerinrust_amd as T
    W, H = X.SIZES[1]

    def cut(T, rt):
        xf = T.MatrixTransformation.create_scaling_matrix(0.0, 1.0, 1.0)
        rt.add_object(rt.csg(rt.sphere((0, 0, 0), 30.0, xf), rt.cube((0, -8, 0), 22.0), "intersection"), T.solid_material((1, 0, 0, 1)))
        rt.add_light((5, 30, -35))

    def plain(T, rt):
        rt.add_object(rt.cube((0, -8, 0), 22.0), T.solid_material((1, 0, 0, 1)))
        rt.add_light((5, 30, -35))
    a, b = _programmatic(W, H, cut), _programmatic(W, H, plain)
    (wa, ia), (wb, ib) = a.tile_masks(), b.tile_masks()
    assert ia["boxed"] == 2 and ib["boxed"] == 2
    assert _bounds(a) == {1: (1, False)} and _bounds(b) == {1: (1, False)}
    assert np.array_equal(wa, wb)
    assert (wa[:, PRIM] & 2 == 0).any() and (wa[:, PRIM] & 2 != 0).any()


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_degenerate_inputs_never_clear_a_bit(size):
    W, H = size

    # a singular leaf transform: the object has no box at all, and its bit stays in every computed word
    def singular(T, rt):
        xf = T.MatrixTransformation.create_scaling_matrix(0.0, 1.0, 1.0)
        rt.add_object(rt.sphere((0, 0, 0), 10.0, xf), T.solid_material((1, 0, 0, 1)))
        rt.add_light((0, 30, -35))
    words, info = _programmatic(W, H, singular).tile_masks()
    assert info["valid"] and not (info["boxed"] >> 1) & 1
    assert ((words >> 1) & 1).all()

    # coordinates beyond RT_CULL_COORD_MAX: an object out there is unboxed, a light out there gives all ones
    def far_object(T, rt):
        xf = T.MatrixTransformation.create_translation_matrix(2.5e6, 0.0, 0.0)
        rt.add_object(rt.sphere((0, 0, 0), 10.0, xf), T.solid_material((1, 0, 0, 1)))
        rt.add_light((0, 30, -35))
    words, info = _programmatic(W, H, far_object).tile_masks()
    assert not (info["boxed"] >> 1) & 1 and ((words >> 1) & 1).all()

    def far_light(T, rt):
        rt.add_object(rt.sphere((0, -5, 0), 12.0), T.solid_material((1, 0, 0, 1)))
        rt.add_light((0, 2.5e6, 0))
        rt.add_light((5, 30, -35))
    words, info = _programmatic(W, H, far_light).tile_masks()
    assert (info["boxed"] >> 1) & 1
    assert (words[:, SHADOW] == ONES).all() and (words[:, SHADOW + 1] != ONES).any()

    # a NaN light (any coordinate): its word is all ones, the other light's is computed
    for k in range(3):
        def nan_light(T, rt):
            p = [0.0, 30.0, -35.0]
            p[k] = math.nan
            rt.add_object(rt.sphere((0, -5, 0), 12.0), T.solid_material((1, 0, 0, 1)))
            rt.add_light(p)
            rt.add_light((5, 30, -35))
        words, info = _programmatic(W, H, nan_light).tile_masks()
        assert (words[:, SHADOW] == ONES).all() and (words[:, SHADOW + 1] != ONES).any()
        assert (words[:, SHADOW + 1] & 2 == 0).any() and (words[:, SHADOW + 1] & 2 != 0).any()
