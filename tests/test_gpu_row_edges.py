"""The row kernels at bisected edges (tests/edge_scenes.py): the generic megakernel, the deferred-shadow kernel, the
wavefront path (wave walk, pairs 1 and 2) render pixel centres only, so the edge suites of
the points kernels never reach their culling walks.  Here the scene is moved to the pixel: every ring scene (the
adjacent doubles of a cube's translation or a light's x between which one pixel's hit signature changes, and their
neighbours) is uploaded and rendered whole at 64x48, depth 4, against the oracle's frame of the same text: RGBA8
equal, f64 within 1e-9 (tests/test_gpu_parity.py assert_close).  One renderer per kernel setting re-uploads scene
after scene; the first-hit points kernel must give the edge pixel's oracle signature in every scene.

The specialised rows are not here: a family program for these scenes (rt_spec_family_register, all of them, the
``s`` scenes alone or the 42 ``l`` scenes alone) is refused by the library's resource guard (rt_spec_rows_00: 1 424 B
of scratch per lane against a bound of 1 024), and a program of its own for each of 206 scenes is 206 compiles.

References are the oracle's alone, computed once per variant and shared (206 frames of 3 072 pixels)."""
import functools

import numpy as np
import pytest

from tests import edge_scenes as E
from tests.test_gpu_first_hits import PLANES, oracle_sample, same_bytes, sample_planes
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEPTH = 4
# (RT_OPT_KERNEL, RT_OPT_WAVEFRONT_PAIRS or None, the last-launch text on an opaque scene, on the glass variant)
SETTINGS = {"mega": ("mega", None, "megakernel", "megakernel"),
            # scenes with a transparent object always take the refraction megakernel (rt_abi.h RT_OPT_KERNEL)
            "deferred": ("deferred", None, "deferred", "megakernel"),
            "wavefront-walk": ("wavefront", 0, "wavefront", "wavefront"),
            "wavefront-pairs1": ("wavefront", 1, "wavefront", "wavefront"),
            "wavefront-pairs2": ("wavefront", 2, "wavefront", "wavefront")}


@functools.lru_cache(maxsize=None)
def reference(variant):
    """Per ring scene of the variant: (edge, value, text, f64 frame, RGBA8 frame, the edge pixel's first-hit planes),
    read-only.  Non-vacuity, from the oracle alone: the frame of an edge's ``lo`` scene and of its ``hi`` scene differ
    at the edge pixel."""
    from oracle import oracle as O
    out, frames = [], {}
    for e, v, text in E.ring_scenes(variant):
        rf, ru = O.OracleScene(text, 0.0, E.W, E.H, max_depth=DEPTH).render(0, E.H, f64=True)
        point = sample_planes([oracle_sample(O.OracleScene(text, 0.0, E.W, E.H, max_depth=0), e.x, e.y)])
        for a in (rf, ru) + tuple(point.values()):
            a.setflags(write=False)
        out.append((e, v, text, rf, ru, point))
        frames[(e, v)] = ru
    seen = sum(bool((frames[(e, e.lo)][e.y, e.x] != frames[(e, e.hi)][e.y, e.x]).any()) for e in E.edges(variant))
    changes = sum(int(a[5]["object"][0]) != int(b[5]["object"][0]) or int(a[5]["shadow"][0]) != int(b[5]["shadow"][0])
                  for a, b in zip(out, out[1:]) if a[0] == b[0])
    # measured: 206 scenes per variant (48 edges: 41 s x 4, 7 l x 6); the edge pixel's RGBA8 differs between the lo
    # and the hi frame at 48 of 48 edges; 66 signature changes between consecutive ring scenes (a ring may hold
    # more than one: next to an edge the signature can flip back within a few doubles)
    print(f"{variant}: {len(out)} ring scenes, {seen} of {len(E.edges(variant))} edges seen in RGBA8, "
          f"{changes} signature changes between consecutive ring scenes")
    assert len(out) >= 4 * 32 and 2 * seen >= len(E.edges(variant)) and changes >= len(E.edges(variant))
    return tuple(out)


def check_scene(T, r, item, label):
    """Upload the item's scene and hold the whole frame, RGBA8 and f64, and the first-hit points kernel at the edge
    pixel, to the oracle's."""
    e, v, text, rf, ru, point = item
    sc = T.Scene.compile(text, 0.0, E.W, E.H)
    r.upload(sc)
    gu = r.render_rows_host(0, E.H, DEPTH)
    info = r.kernel_info()
    gf = r.render_rows_host(0, E.H, DEPTH, f64=True)
    where = f"{label} {e.param}={v!r} edge pixel ({e.x}, {e.y}) [{info}]"
    bad = np.argwhere((gu != ru).any(axis=-1))
    assert len(bad) == 0, (where, [(int(x), int(y), gu[y, x].tolist(), ru[y, x].tolist()) for y, x in bad[:8]])
    assert_close(gu, gf, ru, rf, where)
    got = r.first_hits_points(np.array([[float(e.x), float(e.y)]]), shadow=True, normal=True)
    for k in PLANES:
        assert same_bytes(got[k], point[k]), (where, k, got[k], point[k])
    return info


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("variant", E.VARIANTS)
def test_row_kernels_at_bisected_edges(variant, setting):
    import tinyraytracerinrust_amd as T
    ref = reference(variant)
    kernel, pairs, opaque_says, glass_says = SETTINGS[setting]
    says = glass_says if variant == "glass" else opaque_says
    r = T.Renderer(0, specialize=0)
    r.set_kernel(kernel)
    if pairs is not None:
        r.set_wavefront_pairs(pairs)
    for item in ref:
        info = check_scene(T, r, item, f"{variant} {setting}")
        assert r.kernel_variant() == "generic", info
        assert info.split("last launch: ")[1].split(";")[0] == says, info
    r.free()
