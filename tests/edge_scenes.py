"""Edges for the kernels that take integer pixels only: the scene is moved to the pixel, not the pixel to the scene.

The row kernels (megakernel, deferred-shadow, wavefront wave walk and pairs, the specialised rows) trace pixel
centres, so the bisected sample positions of tests/test_gpu_cull_edges.py never reach them.  Here an integer pixel is
fixed and one number of the scene is bisected until that pixel's hit signature (orc_hit_signature: object and
occluded-light bits) changes between two ADJACENT doubles of the number.  The scene is tests/test_gpu_cull_edges.py's
CUBES at 64x48 with two parameters:

* ``s``: the first cube is drawn under ``translate(repr(s), 0, 0)`` -- its silhouette and its shadows move;
* ``l``: the first appended light stands at x = ``40.0 + l`` (written as its 17-digit repr) -- shadow edges move.

and two variants: "opaque" (reflection-only kernels) and "glass", in which the yellow sphere is transparent and
reflective (``0.2, 0.5``), so a context takes the refraction kernels.  Each edge (lo, hi) yields the four scenes
nextafter(lo, -inf), lo, hi, nextafter(hi, +inf) (an ``l`` edge two more, see ring).  Everything here is computed by
the CPU oracle alone."""
import functools
import math
from collections import namedtuple

W, H = 64, 48
VARIANTS = ("opaque", "glass")
PARAMS = ("s", "l")
MAX_EDGES = 48                       # per variant
LIGHT_X = 40.0
INTERVALS = ((0.0, 6.0), (0.0, -6.0))

Edge = namedtuple("Edge", "param x y lo hi sig_lo sig_hi")


def scene(variant: str, s: float = 0.0, l: float = 0.0) -> str:
    """tests/test_gpu_cull_edges.py CUBES with the two parameters; scene(v) with both 0.0 renders as CUBES does."""
    assert variant in VARIANTS
    sphere = "0.2, 0.5" if variant == "glass" else "0.2"
    return ("draw(plane(<0, 1, 0>, 25, rgb(0.5, 0.5, 0.5), 0.3))\n"
            f"translate({float(s)!r}, 0, 0) draw(cube(<-30, -10, 10>, 14, red, 0.3))\n"
            "draw(cube(<0, -15, 30>, 20, rgb(0.2, 0.8, 0.2), 0.5))\n"
            "translate(25, -5, 0) draw(csg(cube(18), sphere(12), 'intersection', rgb(0.3, 0.3, 0.9), 0.4))\n"
            f"draw(sphere(<10, 10, -10>, 6, rgb(0.9, 0.9, 0.2), {sphere}))\n"
            f"append light(<{LIGHT_X + float(l)!r}, 60, -40>, white * 0.5, 100)\n"
            "append light(<-50, 30, -20>, white * 0.4, 100)\n"
            "set camera(<0, 10, -85>)\n")


def param_scene(variant: str, param: str, v: float) -> str:
    return scene(variant, s=v) if param == "s" else scene(variant, l=v)


def is_silhouette(e: Edge) -> bool:
    """The object changes (a miss counts as one); otherwise only the occluded-light bits do: a shadow edge."""
    return (e.sig_lo % 4096 if e.sig_lo >= 0 else -1) != (e.sig_hi % 4096 if e.sig_hi >= 0 else -1)


def _signature(variant, param, v, x, y):
    from oracle import oracle as O
    return O.OracleScene(param_scene(variant, param, v), 0.0, W, H, max_depth=0).hit_signature(x, y)


def _bisect(variant, param, x, y, lo, hi, s_lo):
    """Adjacent doubles (lo, hi) of the parameter between which pixel (x, y)'s signature leaves s_lo."""
    while math.nextafter(lo, hi) != hi:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if _signature(variant, param, mid, x, y) == s_lo:
            lo = mid
        else:
            hi = mid
    return lo, hi


@functools.lru_cache(maxsize=None)
def candidates(variant: str):
    """Every edge of the step-2 pixel grid: for s and then l, over [0, 6] and then [-6, 0], the pixels whose
    signature differs between the interval's ends, each bisected to adjacent doubles."""
    from oracle import oracle as O
    found = []
    for param in PARAMS:
        for a, b in INTERVALS:
            sa = O.OracleScene(param_scene(variant, param, a), 0.0, W, H, max_depth=0)
            sb = O.OracleScene(param_scene(variant, param, b), 0.0, W, H, max_depth=0)
            for y in range(0, H, 2):
                for x in range(0, W, 2):
                    s0 = sa.hit_signature(x, y)
                    if s0 == sb.hit_signature(x, y):
                        continue
                    lo, hi = sorted(_bisect(variant, param, x, y, a, b, s0))
                    e = Edge(param, x, y, lo, hi, _signature(variant, param, lo, x, y),
                             _signature(variant, param, hi, x, y))
                    # the DSL's numbers are digits with an optional fraction (scene_grammar.pest number_literal): an
                    # edge at 0.0 itself, whose neighbours repr() writes with an exponent, cannot be written
                    if not any("e" in repr(v) for v in ring(e)):
                        found.append(e)
    return tuple(found)


@functools.lru_cache(maxsize=None)
def edges(variant: str):
    """At most MAX_EDGES edges of the variant: silhouettes and shadow edges in equal parts where both kinds allow,
    each kind thinned evenly over its candidates (so both parameters, both intervals and the whole frame stay in)."""
    cand = candidates(variant)
    sil = [e for e in cand if is_silhouette(e)]
    shd = [e for e in cand if not is_silhouette(e)]
    n_sil = min(len(sil), max(MAX_EDGES // 2, MAX_EDGES - len(shd)))
    n_shd = min(len(shd), MAX_EDGES - n_sil)

    def thin(seq, n):
        return [seq[(i * len(seq)) // n] for i in range(n)]
    return tuple(thin(sil, n_sil) + thin(shd, n_shd))


def ring(e: Edge):
    """The four parameter values of an edge: nextafter(lo, -inf), lo, hi, nextafter(hi, +inf).  An ``l`` edge adds
    two: a double of l in [-6, 6] is finer than one of 40.0 + l, so the outer two values mostly round to the light
    positions of the inner two; the added values put the light on the doubles next to those positions (x - 40.0
    and 40.0 + (x - 40.0) are exact for x in [34, 46])."""
    r = (math.nextafter(e.lo, -math.inf), e.lo, e.hi, math.nextafter(e.hi, math.inf))
    if e.param == "l":
        r += (math.nextafter(LIGHT_X + e.lo, -math.inf) - LIGHT_X, math.nextafter(LIGHT_X + e.hi, math.inf) - LIGHT_X)
    return r


@functools.lru_cache(maxsize=None)
def ring_scenes(variant: str):
    """((edge, value, text), ...): every edge's ring scenes."""
    return tuple((e, v, param_scene(variant, e.param, v)) for e in edges(variant) for v in ring(e))
