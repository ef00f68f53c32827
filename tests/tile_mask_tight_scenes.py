"""Scenes for the tighter tile-mask predicate (csrc/rt_tilemask.h vertex sets, ball, clip at the light),
shared by test_tile_masks_tight_host.py and test_gpu_tile_masks_tight.py.  Each scene is the floor plane
plus ONE boxed object, so a floor pixel the oracle finds in shadow names its occluder; the lights are placed
from the object's own world box (rt_scene_describe) at the positions where the clip changes what it does."""
import functools
import re

import numpy as np

SIZES = [(96, 72), (100, 75)]               # the second has a partial tile column and a partial tile row
FLOOR = "draw(plane(<0, 1, 0>, 25.01, rgb(0.6, 0.6, 0.6), 0.3))\n"
CAMERA = "set camera(<0, 10, -85>)\n"

# object 1 of every scene (object 0 is the floor)
OBJECTS = {
    # a thin rod tilted about two axes: a sphere scaled (1, 100, 1) cut to length by a cube (globes.scene's rods)
    "rod": """
translate(4, -2, 6)
rotate(0.5, 0, 0.35) do
  scale(1, 100, 1)
    a = sphere(1)
  rod = csg(a, cube(36), 'intersection', red, 0.2)
end
draw(rod)
""",
    # a thin tilted slab: a cube scaled 0.05 along x
    "slab": """
translate(-6, -4, 8)
rotate(0.25, 0.6, 0.3) do
  scale(0.05, 1, 1)
    s = cube(30, green, 0.2)
end
draw(s)
""",
    "sphere": "draw(sphere(<-8, -3, 5>, 13, red, 0.3))\n",
    # a CSG difference shell: only the outer sphere bounds its hits
    "shell": """
outer = sphere(<3, -4, 0>, 14)
inner = sphere(<3, -4, 0>, 12)
draw(csg(outer, inner, 'difference', yellow, 0.2))
""",
    # the required leaf (the sphere) is not the object's smallest box (the cube that is cut out of it)
    "bitten": """
a = sphere(<0, -5, 0>, 14)
b = cube(<7, 0, -7>, 9)
draw(csg(a, b, 'difference', blue, 0.2))
""",
    # a cube cut round by a sphere scaled (1, 100000, 1): the sphere leaf's own box reaches 1.5e6, beyond
    # RT_CULL_COORD_MAX, so its vertex set must be dropped while the object keeps the cube's finite bounds
    "column": """
b = cube(<2, -8, 4>, 22)
scale(1, 100000, 1)
  a = sphere(<2, 0, 4>, 15)
draw(csg(a, b, 'intersection', red, 0.2))
""",
    # a sphere under a non-similarity: an ellipsoid, which has a vertex set and must take no ball
    "ellipsoid": """
translate(5, -3, 0)
rotate(0, 0, 0.4) do
  scale(1, 2.5, 0.8)
    e = sphere(7, red, 0.2)
end
draw(e)
""",
}


def _text(obj, lights):
    return FLOOR + OBJECTS[obj] + "".join(f"append light(<{x!r}, {y!r}, {z!r}>, white * 0.4, 100)\n" for x, y, z in lights) + CAMERA


@functools.lru_cache(maxsize=None)
def object_box(obj):
    """World box (lo, hi) of the scene's object 1, as the flattener has it."""
    import tinyraytracerinrust_amd as T
    d = T.Scene.compile(_text(obj, ()), 0.0, 96, 72).describe()
    m = re.search(r"object 1 cull=1 box \[(\S+) (\S+) (\S+)\]\.\.\[(\S+) (\S+) (\S+)\]", d)
    assert m, d
    v = [float(g) for g in m.groups()]
    return v[:3], v[3:]


def lights(obj):
    """Two groups (with the default light each scene stays within the predicate's four): lower than the
    object's top, above it, beside it; exactly at the top's height, and with x on a face of the box."""
    lo, hi = object_box(obj)
    cx, cz, top = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[2] + hi[2]), hi[1]
    mid = 0.5 * (max(lo[1], -25.0) + top)
    return {"low_above_beside": [(cx + 5.0, mid, cz - 35.0), (cx - 8.0, top + 25.0, cz - 30.0), (hi[0] + 30.0, mid, cz)],
            "top_face": [(cx + 12.0, top, cz - 25.0), (hi[0], top + 10.0, cz - 20.0)]}


def scenes():
    """name -> scene text"""
    out = {}
    for obj in OBJECTS:
        for group, ls in lights(obj).items():
            out[f"{obj}-{group}"] = _text(obj, tuple(ls))
    return out


@functools.lru_cache(maxsize=None)
def signatures(name, W, H):
    """orc_hit_signature of every pixel: int64 [H, W] (-1 miss, else object + 1 + 4096 * occluded lights)."""
    from oracle import oracle as O
    sc = O.OracleScene(scenes()[name], 0.0, W, H)
    sig = np.empty((H, W), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            sig[y, x] = sc.hit_signature(x, y)
    return sig


def world_box_walks(sc, W, H, pn=(0.0, 1.0, 0.0), pd=25.01):
    """The predicate with the objects' world boxes alone (8 corners against the cone's and the pyramids' side
    planes, the planes parallel to the mask plane, the AABB of the floor patch and the light; no vertex sets,
    no ball, no clip), restated in numpy for a whole-frame launch of scene `sc` whose mask plane is
    pn . x + pd = 0: per tile the sets of boxed objects left in (prim, [shadow per light] or None, refl or None).
    Tolerances are left out: they move no count."""
    boxes = {}
    for m in re.finditer(r"object (\d+) cull=1 box \[(\S+) (\S+) (\S+)\]\.\.\[(\S+) (\S+) (\S+)\]", sc.describe()):
        v = [float(g) for g in m.groups()[1:]]
        boxes[int(m.group(1))] = np.array([[v[3 + i] if (k >> i) & 1 else v[i] for i in range(3)] for k in range(8)])
    cam = sc.camera()
    C, D, R, U = (np.array(cam[k], dtype=float) for k in ("center", "direction", "right", "up"))
    lights = [np.array(sc.light(i)[0], dtype=float) for i in range(sc.info()["lights"])]
    pn = np.array(pn, dtype=float)

    def side_planes(v):
        vc, out = v.sum(axis=0), []
        for i in range(4):
            m = np.cross(v[i], v[(i + 1) & 3])
            s = m @ vc
            if s == 0.0:
                return None
            m = -m if s < 0 else m
            if not (m @ v[(i + 2) & 3] > 0 and m @ v[(i + 3) & 3] > 0):
                return None
            out.append(m)
        return out

    def outside(o, n, apex):
        return bool((((boxes[o] - apex) @ n) < 0).all())

    tiles = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            xs = (tx * 8 - 0.5, min(tx * 8 + 7, W - 1) + 0.5)
            ys = (ty * 8 - 0.5, min(ty * 8 + 7, H - 1) + 0.5)
            d = np.array([D + R * (((xs[1 if k in (1, 2) else 0] / W) - 0.5) * cam["aspect"]) +
                          U * ((H - 1.0 - ys[1 if k >= 2 else 0]) / H - 0.5) for k in range(4)])
            n = side_planes(d)
            if n is None:
                tiles.append((set(boxes), None, None))
                continue
            prim = {o for o in boxes if not any(outside(o, ni, C) for ni in n)}
            sC, vd = pn @ C + pd, d @ pn
            if not ((vd * sC < 0).all() and (vd * vd >= 1e-8 * (pn @ pn) * (d * d).sum(axis=1)).all()):
                tiles.append((prim, None, None))
                continue
            Q = C + d * (-sC / vd)[:, None]
            shadow = []
            for L in lights:
                sL = pn @ L + pd
                up = pn if sL > 0 else -pn
                m = side_planes(Q - L)
                lo, hi = np.minimum(Q.min(axis=0), L), np.maximum(Q.max(axis=0), L)
                keep = set()
                for o, c in boxes.items():
                    cull = outside(o, up, Q[0]) or outside(o, -up, L) or bool((c.min(axis=0) > hi).any() or (c.max(axis=0) < lo).any())
                    cull = cull or (m is not None and any(outside(o, mi, L) for mi in m))
                    if not cull:
                        keep.add(o)
                shadow.append(keep)
            Cm = C - pn * (2.0 * sC / (pn @ pn))
            m = side_planes(Q - Cm)
            cs = pn if sC > 0 else -pn
            refl = {o for o in boxes if not ((m is not None and any(outside(o, mi, Cm) for mi in m)) or outside(o, cs, Q[0]))}
            tiles.append((prim, shadow, refl))
    return tiles
