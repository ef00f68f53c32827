"""Bisected silhouette and shadow edges through the first-hit points kernel (rt_first_hits_points).

The first-hit maps are the sharpest probe of the culling walks there is: a wrongly culled box changes the object id
or a shadow bit outright, where a colour may or may not move a channel.  The points are tests/test_gpu_cull_edges.py's:
along scan lines in both directions every change of the oracle's hit signature is bisected to adjacent doubles of
the sample position, and the 8 doubles around each edge are sampled.  The reference is oracle_sample per point (the
oracle's two paths, cross-checked); object, occluded-light mask, the distance's bytes and the raw normal's bytes
must all be equal."""
import functools
import math

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.test_gpu_cull_edges import CUBES, _edges
from tests.test_gpu_first_hits import PLANES, check_misses, oracle_sample, sample_planes

pytestmark = pytest.mark.gpu

RING = 8
CASES = [("cubes", 0.0, 1920, 1080),               # axis-aligned cubes: boxes that ARE the surfaces
         ("spinning_globes", 0.5, 1920, 1080),     # glass shells: the REFR walks (shared sphere terms)
         ("three_cubes", 0.0, 1920, 1080),         # rotated cubes: oriented object boxes
         ("globes", 0.0, 3840, 2160)]              # the headline frame


def text_of(name):
    return CUBES if name == "cubes" else scene_text(name)


@functools.lru_cache(maxsize=None)
def reference(name, t, W, H):
    """(points (n, 2), the four planes of oracle_sample at each, object-changing pairs, mask-only pairs), read-only.
    The pairs are counted between neighbours within each ring of 8 doubles."""
    from oracle import oracle as O
    osc = O.OracleScene(text_of(name), t, W, H, max_depth=0)
    pts = []
    for along_x in (True, False):
        for lo, hi, c in _edges(osc, W, H, along_x, n_lines=80, step=2.0, cap=200):
            ring = [lo, hi]
            for _ in range(3):                                # 3 more doubles on each side
                ring = [math.nextafter(ring[0], -math.inf)] + ring + [math.nextafter(ring[-1], math.inf)]
            pts += [(p, c) if along_x else (c, p) for p in ring]
    xy = np.array(pts, dtype=np.float64)
    ref = sample_planes([oracle_sample(osc, x, y) for x, y in pts])
    check_misses(ref)
    obj, mask = ref["object"].reshape(-1, RING), ref["shadow"].reshape(-1, RING)
    d_obj = obj[:, 1:] != obj[:, :-1]
    d_mask = ~d_obj & (mask[:, 1:] != mask[:, :-1])
    print(f"{name} t={t} {W}x{H}: {len(pts)} points at {len(pts) // RING} edges; neighbours that differ in object "
          f"{int(d_obj.sum())}, in mask only {int(d_mask.sum())}; misses {int((ref['object'] < 0).sum())}")
    for a in (xy,) + tuple(ref.values()):
        a.setflags(write=False)
    return xy, ref, int(d_obj.sum()), int(d_mask.sum())


@pytest.mark.parametrize("name,t,W,H", CASES)
def test_first_hits_at_bisected_edges(worldmap, name, t, W, H):
    import tinyraytracerinrust_amd as T
    xy, ref, n_obj, n_mask = reference(name, t, W, H)
    # measured (points at edges; neighbours that differ in object; in mask only): cubes 2 744 at 343; 170; 254 --
    # spinning_globes 2 176 at 272; 245; 139 -- three_cubes 2 920 at 365; 234; 144 -- globes 2 720 at 340; 177; 246
    # (a ring can hold more than one change: next to an edge the signature may flip back within a few doubles)
    assert len(xy) >= 1200, len(xy)
    assert n_obj >= 100 and n_mask >= 50, (n_obj, n_mask)
    r = T.Renderer(0)
    r.upload(T.Scene.compile(text_of(name), t, W, H, asset_dir=SCENES))
    got = r.first_hits_points(xy, shadow=True, normal=True)
    n = len(xy)
    differ = {k: (np.ascontiguousarray(got[k]).view(np.uint8).reshape(n, -1) !=
                  np.ascontiguousarray(ref[k]).view(np.uint8).reshape(n, -1)).any(axis=1) for k in PLANES}
    print(f"{name}: points that differ per plane { {k: int(v.sum()) for k, v in differ.items()} }")
    bad = np.nonzero(np.any(list(differ.values()), axis=0))[0]

    def signature(p, i):
        return (int(p["object"][i]), hex(int(p["shadow"][i])), float(p["distance"][i]).hex(),
                [float(c).hex() for c in p["normal"][i]])
    assert len(bad) == 0, (f"{len(bad)} of {n} points differ; kernel: {r.kernel_info()}",
                           [(tuple(xy[i].tolist()), "gpu", signature(got, i), "oracle", signature(ref, i))
                            for i in bad[:8]])
    for k in PLANES:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    # the kernel without a shadow walk and without normals: the same objects and distances
    lean = r.first_hits_points(xy)
    assert set(lean) == {"object", "distance"}
    assert lean["object"].tobytes() == ref["object"].tobytes() and lean["distance"].tobytes() == ref["distance"].tobytes()
