"""Scenes, sizes and launch geometries shared by the tile-mask tests (test_tile_masks_host.py on the CPU,
test_gpu_tile_masks.py on the GPU), and the per-pixel oracle signatures both check masks against."""
import functools

import numpy as np

from tests.conftest import scene_text

SIZES = [(96, 72), (203, 117)]              # neither width nor height a multiple of the 8x8 tile
BAND, WORLD = 8, 3                          # the cyclic band layout: bands of 8 rows dealt to 3 ranks

# every scene also holds the default light at (-10, 30, -50) (RayTracer::add_test_objects)
_CUBES_CSG = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(cube(<-30, -15, 10>, 20, red))
draw(cube(<25, -17, -20>, 16, blue, 0.4))
draw(cube(<0, -20, 40>, 10, green))
a = sphere(<0, -5, 0>, 14)
b = cube(<6, -5, -6>, 16)
draw(csg(a, b, 'difference', yellow, 0.2))
append light(<40, 20, -35>, white * 0.4, 100)
append light(<-5, 60, 30>, white * 0.3, 100)
set camera(<0, 10, -85>)
"""
_TILTED = """
draw(plane(<0.2, 1, -0.1>, 30, rgb(0.5, 0.5, 0.7), 0.4))
draw(sphere(<-10, 0, 0>, 12, red))
draw(cube(<20, -5, 10>, 14, green, 0.3))
append light(<0, 40, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
# a plane leaf under a non-identity transform: rotated about two axes and translated (the mask plane's
# world-space form comes from the leaf's inverse transform)
_XF_PLANE = """
translate(5, -8, 12)
rotate(0.15, 0.4, -0.1)
  draw(plane(<0, 1, 0>, 22, rgb(0.5, 0.6, 0.5), 0.4))
draw(sphere(<-12, 0, 0>, 12, red))
draw(cube(<22, -4, 15>, 14, blue, 0.3))
append light(<5, 45, -30>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
_LIGHT_BELOW = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<0, -5, 0>, 15, red))
draw(cube(<-30, -40, 0>, 12, blue))
append light(<10, -60, -20>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
_CAMERA_BELOW = """
draw(plane(<0, 1, 0>, -30, rgb(0.6, 0.6, 0.6), 0.5))
draw(sphere(<0, 5, 0>, 15, red))
draw(cube(<-30, 10, 20>, 12, blue))
append light(<10, -10, -60>, white * 0.5, 100)
set camera(<0, 0, -85>)
"""
_TWO_PLANES = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(plane(<0, 0, -1>, 120, rgb(0.3, 0.5, 0.3), 0.2))
draw(sphere(<-15, -5, 0>, 14, red))
draw(cube(<25, -15, 20>, 18, blue))
append light(<0, 20, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
_NO_PLANE = """
draw(sphere(<-15, -5, 0>, 14, red, 0.3))
draw(cube(<25, -15, 20>, 18, blue))
append light(<0, 20, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""
_FIVE_LIGHTS = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
draw(sphere(<-15, -5, 0>, 14, red))
draw(cube(<25, -15, 20>, 18, blue))
append light(<0, 20, -35>, white * 0.2, 100)
append light(<30, 20, -35>, white * 0.2, 100)
append light(<-30, 20, -35>, white * 0.2, 100)
append light(<0, 50, 35>, white * 0.2, 100)
set camera(<0, 10, -85>)
"""
_CAMERA_IN_BOX = """
draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))
big = cube(<0, 10, -85>, 60)
hole = sphere(<0, 10, -85>, 36)
draw(csg(big, hole, 'difference', rgb(0.4, 0.4, 0.8), 0.2))
draw(sphere(<0, -5, 0>, 15, red))
append light(<0, 20, -35>, white * 0.5, 100)
set camera(<0, 10, -85>)
"""


def scenes():
    """name -> (scene text, time)"""
    return {
        "globes": (scene_text("globes"), 0.0),
        "three_cubes": (scene_text("three_cubes"), 0.0),
        "ground_star": (scene_text("ground_star"), 0.0),
        "cubes_csg_3lights": (_CUBES_CSG, 0.0),
        "tilted_plane": (_TILTED, 0.0),
        "transformed_plane": (_XF_PLANE, 0.0),
        "light_below": (_LIGHT_BELOW, 0.0),
        "camera_below": (_CAMERA_BELOW, 0.0),
        "two_planes": (_TWO_PLANES, 0.0),
        "no_plane": (_NO_PLANE, 0.0),
        "five_lights": (_FIVE_LIGHTS, 0.0),
        "camera_in_box": (_CAMERA_IN_BOX, 0.0),
    }


def geometries(H):
    """(label, y_first, band_rows, band_pitch, n_bands): the whole frame, then each rank's cyclic bands."""
    from tinyraytracerinrust_amd import distributed as D
    out = [("frame", 0, H, H, 1)]
    for rank in range(WORLD):
        out.append((f"rank{rank}",) + tuple(D.band_params(H, WORLD, rank, "cyclic", BAND)))
    return out


def frame_rows(H, y_first, band_rows, band_pitch, n_bands):
    """Output row r -> frame row y (or -1 past the frame), as rt_device.h band_row."""
    n_rows = band_rows * n_bands
    r = np.arange(n_rows)
    y = y_first + r if band_rows >= n_rows else y_first + (r // band_rows) * band_pitch + r % band_rows
    return np.where(y < H, y, -1)


@functools.lru_cache(maxsize=None)
def signatures(name, W, H):
    """orc_hit_signature of every pixel: int64 [H, W] (-1 miss, else object + 1 + 4096 * occluded lights)."""
    from oracle import oracle as O
    import os
    from tests.conftest import SCENES
    O.register_texture_file("worldmap.png", os.path.join(SCENES, "worldmap.png"))
    text, t = scenes()[name]
    sc = O.OracleScene(text, t, W, H)
    sig = np.empty((H, W), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            sig[y, x] = sc.hit_signature(x, y)
    return sig
