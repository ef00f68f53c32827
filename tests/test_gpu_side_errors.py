"""The side entries' refusals as one table: every row is one call through the C ABI that must be refused (or, where
marked, accepted without work) with exactly this status AND exactly this rt_last_error() text.  The entries are those
around the row loop: sample points, first hits, ray counts, ray paths and the single-sample recorder, the three
anti-aliasing entries, the orthogonal views and the two frame assemblies.  Where one call trips two checks the row
pins which check answers.  No refused call may touch its buffers.

Three 24x13 `globes` contexts -- perspective (P), stereoscopic (S), anaglyph (A) -- and one without a scene (E)."""
import ctypes
import types

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text

pytestmark = pytest.mark.gpu

W, H = 24, 13
OK, INVALID, UNSUPPORTED = 0, -1, -6
NAN = float("nan")
NO_SCENE = "no scene uploaded to this context"
NULL = "null argument"
DEPTH = "max_depth 17 > 16"
ROW4, ROW16, ROW32 = W * 4, W * 16, W * 32             # 96, 384, 768


def two_eye(who):
    return f"{who} is not built for a two-eye scene (stereoscopic / anaglyph camera)"


@pytest.fixture(scope="module")
def env(worldmap):
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = types.SimpleNamespace(T=T, lib=T.lib(), keep=[])
    for name, kind in (("P", None), ("S", "stereoscopic"), ("A", "anaglyph")):
        sc = T.Scene.compile(scene_text("globes"), 0.0, W, H, asset_dir=SCENES)
        if kind:
            sc.set_camera_kind(kind, 4.0)
        r = T.Renderer(0)
        r.upload(sc)
        e.keep += [sc, r]
        setattr(e, name, r.h)
    empty = T.Renderer(0)
    e.keep.append(empty)
    e.E = empty.h
    e.buf = np.full(W * H * 32 + 64, 0xA5, np.uint8)    # any argument's memory: a whole f64 frame and some
    e.B = e.buf.ctypes.data
    assert e.B % 16 == 0
    e.n32 = ctypes.c_int32(-7)
    e.n64 = ctypes.c_uint64(7)
    e.u32 = ctypes.c_uint32(7)
    e.counts = _lib_struct(T, "rt_ray_counts")
    return e


def _lib_struct(T, name):
    from tinyraytracerinrust_amd import _lib
    return getattr(_lib, name)()


def planes(e, object_stride=ROW4, none=False):
    """rt_hit_planes asking for the object plane alone (none: for nothing)."""
    from tinyraytracerinrust_amd import _lib
    p = _lib.rt_hit_planes()
    if not none:
        p.object, p.object_stride = e.B, object_stride
    return ctypes.byref(p)


def aa(e, c, src=True, th=0.01, level=2, depth=-1, sstride=ROW4, dst=True, dstride=ROW4, f64=False, fstride=ROW32):
    return (c, e.B if src else None, sstride, th, level, depth, e.B if dst else None, dstride, e.B if f64 else None, fstride,
            ctypes.byref(e.n64), None)


def aab(e, c, bands=(0, 8, 8, 1), src=True, th=0.01, level=2, depth=-1, sstride=ROW4, dst=True, dstride=ROW4, f64=False,
        fstride=ROW32):
    return (c, e.B if src else None, sstride, th, level, depth) + tuple(bands) + (
        e.B if dst else None, dstride, e.B if f64 else None, fstride, ctypes.byref(e.n64), None)


def ortho(e, c, a1=0, a2=1, y0=0, y1=H, u8=True, stride=ROW4, f64=False, fstride=ROW32):
    return (c, a1, a2, 1.0, 1.0, 1.0, y0, y1, e.B if u8 else None, stride, e.B if f64 else None, fstride, None)


def asm(e, g=True, gstride=ROW4, world=2, slot=8, band=2, height=H, row=ROW4, f=0, fstride=ROW4):
    """Both assemblies' arguments (row: row_bytes, or the width for the RGB8 entry); f: the frame's byte offset."""
    return (e.B if g else None, gstride, world, slot, band, height, row, e.B + 4096 + f, fstride, None)


# (id, entry, arguments from the environment, status, rt_last_error() text)
ROWS = [
    # ------------------------------------------------------------ k_points
    ("points-null-out", "rt_render_points_f64", lambda e: (e.P, e.B, 1, -1, None, None), INVALID, NULL),
    ("points-null-before-upload", "rt_render_points_f64", lambda e: (e.E, None, 1, -1, e.B, None), INVALID, NULL),
    ("points-no-upload", "rt_render_points_f64", lambda e: (e.E, e.B, 1, -1, e.B, None), INVALID, NO_SCENE),
    ("points-upload-before-depth", "rt_render_points_f64", lambda e: (e.E, e.B, 1, 17, e.B, None), INVALID, NO_SCENE),
    ("points-depth", "rt_render_points_f64", lambda e: (e.P, e.B, 1, 17, e.B, None), UNSUPPORTED, DEPTH),
    ("points-depth-before-empty", "rt_render_points_f64", lambda e: (e.P, e.B, 0, 17, e.B, None), UNSUPPORTED, DEPTH),
    ("points-depth-two-eye", "rt_render_points_f64", lambda e: (e.S, e.B, 1, 17, e.B, None), UNSUPPORTED, DEPTH),
    ("pixel-null-scene", "rt_trace_pixel_f64", lambda e: (None, 1.0, 1.0, -1, 0, e.B), INVALID, NULL),
    # ------------------------------------------------------------ k_hits
    ("hits-bands-null", "rt_first_hits_row_bands", lambda e: (e.P, 0, 8, 8, 1, planes(e, none=True), None), INVALID, NULL),
    ("hits-bands-null-before-upload", "rt_first_hits_row_bands", lambda e: (e.E, 0, 8, 8, 1, None, None), INVALID, NULL),
    ("hits-bands-no-upload", "rt_first_hits_row_bands", lambda e: (e.E, 0, 8, 8, 1, planes(e), None), INVALID, NO_SCENE),
    ("hits-bands-anaglyph", "rt_first_hits_row_bands", lambda e: (e.A, 0, 8, 8, 1, planes(e), None), UNSUPPORTED,
     "first hits of an anaglyph scene: a pixel has two, one per eye"),
    ("hits-bands-anaglyph-before-stride", "rt_first_hits_row_bands", lambda e: (e.A, 0, 8, 8, 1, planes(e, ROW4 - 4), None),
     UNSUPPORTED, "first hits of an anaglyph scene: a pixel has two, one per eye"),
    ("hits-bands-stride", "rt_first_hits_row_bands", lambda e: (e.P, 0, 8, 8, 1, planes(e, ROW4 - 4), None), INVALID,
     "object stride 92 < 96"),
    ("hits-bands-stride-before-bands", "rt_first_hits_row_bands", lambda e: (e.P, H, 8, 8, 1, planes(e, ROW4 - 4), None),
     INVALID, "object stride 92 < 96"),
    ("hits-bands-first-row", "rt_first_hits_row_bands", lambda e: (e.S, H, 8, 8, 1, planes(e), None), INVALID,
     "first row 13 >= height 13"),
    ("hits-no-upload", "rt_first_hits", lambda e: (e.E, 5, 3, planes(e), None), INVALID, NO_SCENE),
    ("hits-null", "rt_first_hits", lambda e: (e.E, 0, H, planes(e, none=True), None), INVALID, NULL),
    ("hits-row-range", "rt_first_hits", lambda e: (e.P, 5, 3, planes(e), None), INVALID, "bad row range [5, 3) for height 13"),
    ("hits-row-range-before-anaglyph", "rt_first_hits", lambda e: (e.A, 0, H + 1, planes(e), None), INVALID,
     "bad row range [0, 14) for height 13"),
    ("hits-anaglyph", "rt_first_hits", lambda e: (e.A, 0, H, planes(e), None), UNSUPPORTED,
     "first hits of an anaglyph scene: a pixel has two, one per eye"),
    ("hits-points-null", "rt_first_hits_points", lambda e: (e.P, None, 1, e.B, None, None, None, None), INVALID, NULL),
    ("hits-points-no-outputs", "rt_first_hits_points", lambda e: (e.E, e.B, 1, None, None, None, None, None), INVALID, NULL),
    ("hits-points-no-upload", "rt_first_hits_points", lambda e: (e.E, e.B, 1, e.B, None, None, None, None), INVALID, NO_SCENE),
    ("hits-points-anaglyph-before-count", "rt_first_hits_points", lambda e: (e.A, e.B, 1 << 31, e.B, None, None, None, None),
     UNSUPPORTED, "first hits of an anaglyph scene: a pixel has two, one per eye"),
    ("hits-points-too-many", "rt_first_hits_points", lambda e: (e.S, e.B, 1 << 31, e.B, None, None, None, None), INVALID,
     "2147483648 sample positions > 2147483647"),
    # ------------------------------------------------------------ k_stats
    ("count-bands-null", "rt_count_rays_row_bands", lambda e: (e.E, 0, 8, 8, 1, -1, None, None, None, 0, None), INVALID, NULL),
    ("count-bands-no-upload", "rt_count_rays_row_bands",
     lambda e: (e.E, 0, 8, 8, 1, 17, ctypes.byref(e.counts), None, None, 0, None), INVALID, NO_SCENE),
    ("count-bands-depth", "rt_count_rays_row_bands",
     lambda e: (e.S, 0, 8, 8, 1, 17, ctypes.byref(e.counts), None, None, 0, None), UNSUPPORTED, DEPTH),
    ("count-bands-depth-before-stride", "rt_count_rays_row_bands",
     lambda e: (e.P, 0, 8, 8, 1, 17, None, None, e.B, ROW16 - 4, None), UNSUPPORTED, DEPTH),
    ("count-bands-stride", "rt_count_rays_row_bands", lambda e: (e.P, 0, 8, 8, 1, -1, None, None, e.B, ROW16 - 4, None),
     INVALID, "pixel stride 380 < 384"),
    ("count-bands-stride-before-bands", "rt_count_rays_row_bands",
     lambda e: (e.P, H, 8, 8, 1, -1, None, None, e.B, ROW16 - 4, None), INVALID, "pixel stride 380 < 384"),
    ("count-bands-pitch", "rt_count_rays_row_bands", lambda e: (e.P, 0, 8, 4, 2, -1, None, None, e.B, ROW16, None),
     INVALID, "band pitch 4 < band rows 8"),
    ("count-null", "rt_count_rays", lambda e: (e.E, 5, 3, -1, None, None, None, 0, None), INVALID, NULL),
    ("count-no-upload", "rt_count_rays", lambda e: (e.E, 5, 3, 17, None, None, e.B, ROW16, None), INVALID, NO_SCENE),
    ("count-row-range-before-depth", "rt_count_rays", lambda e: (e.P, 5, 3, 17, None, None, e.B, ROW16, None), INVALID,
     "bad row range [5, 3) for height 13"),
    ("count-depth", "rt_count_rays", lambda e: (e.P, 0, H, 17, None, None, e.B, ROW16, None), UNSUPPORTED, DEPTH),
    # ------------------------------------------------------------ k_paths
    ("offsets-null-offsets", "rt_ray_paths_offsets", lambda e: (e.P, e.B, 1, -1, None, None, None), INVALID, NULL),
    ("offsets-null-ctx", "rt_ray_paths_offsets", lambda e: (None, e.B, 1, -1, e.B, None, None), INVALID, NULL),
    ("offsets-no-upload", "rt_ray_paths_offsets", lambda e: (e.E, e.B, 1, 17, e.B, None, None), INVALID, NO_SCENE),
    ("offsets-two-eye-before-depth", "rt_ray_paths_offsets", lambda e: (e.S, e.B, 1, 17, e.B, None, None), UNSUPPORTED,
     two_eye("rt_ray_paths_offsets")),
    ("offsets-depth-before-count", "rt_ray_paths_offsets", lambda e: (e.P, e.B, (1 << 26) + 1, 17, e.B, None, None),
     UNSUPPORTED, DEPTH),
    ("offsets-too-many-before-null-xy", "rt_ray_paths_offsets", lambda e: (e.P, None, (1 << 26) + 1, -1, e.B, None, None),
     UNSUPPORTED, "67108865 sample positions > 67108864"),
    ("offsets-null-xy", "rt_ray_paths_offsets", lambda e: (e.P, None, 1, -1, e.B, None, None), INVALID, NULL),
    ("paths-null-ctx", "rt_ray_paths", lambda e: (None, e.B, 1, -1, e.B, e.B, 1, None, None), INVALID, NULL),
    ("paths-no-upload-before-null-offsets", "rt_ray_paths", lambda e: (e.E, e.B, 1, -1, None, e.B, 1, None, None),
     INVALID, NO_SCENE),
    ("paths-two-eye", "rt_ray_paths", lambda e: (e.A, e.B, 1, 17, e.B, e.B, 1, None, None), UNSUPPORTED, two_eye("rt_ray_paths")),
    ("paths-depth", "rt_ray_paths", lambda e: (e.P, e.B, 1, 17, e.B, e.B, 1, None, None), UNSUPPORTED, DEPTH),
    ("paths-too-many", "rt_ray_paths", lambda e: (e.P, e.B, (1 << 26) + 1, -1, e.B, e.B, 1, None, None), UNSUPPORTED,
     "67108865 sample positions > 67108864"),
    ("paths-null-xy", "rt_ray_paths", lambda e: (e.P, None, 1, -1, None, e.B, 1, None, None), INVALID, NULL),
    ("paths-empty-before-null-offsets", "rt_ray_paths", lambda e: (e.P, None, 0, -1, None, None, 1, None, None), OK, None),
    ("paths-null-offsets", "rt_ray_paths", lambda e: (e.P, e.B, 1, -1, None, e.B, 1, None, None), INVALID, NULL),
    ("paths-null-records", "rt_ray_paths", lambda e: (e.P, e.B, 1, -1, e.B, None, 1, None, None), INVALID, NULL),
    # ------------------------------------------------------------ the single-sample recorder
    ("record-null-count", "rt_record_rays", lambda e: (e.P, 1.0, 1.0, -1, e.B, 4, None, None), INVALID, NULL),
    ("record-null-records", "rt_record_rays", lambda e: (e.P, 1.0, 1.0, -1, None, 4, ctypes.byref(e.n32), None), INVALID, NULL),
    ("record-negative-cap", "rt_record_rays", lambda e: (e.E, 1.0, 1.0, -1, e.B, -1, ctypes.byref(e.n32), None), INVALID, NULL),
    ("record-no-upload", "rt_record_rays", lambda e: (e.E, 1.0, 1.0, 17, e.B, 4, ctypes.byref(e.n32), None), INVALID, NO_SCENE),
    ("record-two-eye-before-depth", "rt_record_rays", lambda e: (e.S, 1.0, 1.0, 17, e.B, 4, ctypes.byref(e.n32), None),
     UNSUPPORTED, two_eye("rt_record_rays")),
    ("record-depth", "rt_record_rays", lambda e: (e.P, 1.0, 1.0, 17, e.B, 4, ctypes.byref(e.n32), None), UNSUPPORTED, DEPTH),
    # ------------------------------------------------------------ anti-aliasing
    ("aa-null-src", "rt_antialias", lambda e: aa(e, e.E, src=False), INVALID, NULL),
    ("aa-null-outputs", "rt_antialias", lambda e: aa(e, e.P, dst=False), INVALID, NULL),
    ("aa-no-upload", "rt_antialias", lambda e: aa(e, e.E, level=5), INVALID, NO_SCENE),
    ("aa-two-eye-before-level", "rt_antialias", lambda e: aa(e, e.S, level=5), UNSUPPORTED, two_eye("rt_antialias")),
    ("aa-level", "rt_antialias", lambda e: aa(e, e.P, level=5), UNSUPPORTED, "anti-aliasing level 5 > 4"),
    ("aa-level-before-nan", "rt_antialias", lambda e: aa(e, e.P, level=5, th=NAN), UNSUPPORTED, "anti-aliasing level 5 > 4"),
    ("aa-nan", "rt_antialias", lambda e: aa(e, e.P, th=NAN), INVALID, "threshold is NaN"),
    ("aa-nan-before-depth", "rt_antialias", lambda e: aa(e, e.P, th=NAN, depth=17), INVALID, "threshold is NaN"),
    ("aa-depth", "rt_antialias", lambda e: aa(e, e.P, depth=17), UNSUPPORTED, DEPTH),
    ("aa-depth-before-stride", "rt_antialias", lambda e: aa(e, e.P, depth=17, sstride=ROW4 - 4), UNSUPPORTED, DEPTH),
    ("aa-source-stride", "rt_antialias", lambda e: aa(e, e.P, sstride=ROW4 - 4, dstride=ROW4 - 4), INVALID, "source stride 92 < 96"),
    ("aa-output-stride", "rt_antialias", lambda e: aa(e, e.P, dstride=ROW4 - 4, f64=True, fstride=ROW32 - 8), INVALID,
     "output stride 92 < 96"),
    ("aa-f64-stride", "rt_antialias", lambda e: aa(e, e.P, f64=True, fstride=ROW32 - 8), INVALID, "f64 stride 760 < 768"),
    ("aa-output-stride-unasked", "rt_antialias", lambda e: aa(e, e.P, dst=False, dstride=0, f64=True, fstride=ROW32 - 8),
     INVALID, "f64 stride 760 < 768"),
    ("aab-null-src", "rt_antialias_row_bands", lambda e: aab(e, e.P, src=False), INVALID, NULL),
    ("aab-no-upload", "rt_antialias_row_bands", lambda e: aab(e, e.E, th=NAN), INVALID, NO_SCENE),
    ("aab-two-eye", "rt_antialias_row_bands", lambda e: aab(e, e.A, th=NAN), UNSUPPORTED, two_eye("rt_antialias_row_bands")),
    ("aab-level", "rt_antialias_row_bands", lambda e: aab(e, e.P, level=5, depth=17), UNSUPPORTED, "anti-aliasing level 5 > 4"),
    ("aab-nan", "rt_antialias_row_bands", lambda e: aab(e, e.P, th=NAN, sstride=0), INVALID, "threshold is NaN"),
    ("aab-depth", "rt_antialias_row_bands", lambda e: aab(e, e.P, depth=17, bands=(H, 8, 8, 1)), UNSUPPORTED, DEPTH),
    ("aab-source-stride", "rt_antialias_row_bands", lambda e: aab(e, e.P, sstride=ROW4 - 1), INVALID, "source stride 95 < 96"),
    ("aab-output-stride", "rt_antialias_row_bands", lambda e: aab(e, e.P, dstride=ROW4 - 4), INVALID, "output stride 92 < 96"),
    ("aab-f64-stride-before-bands", "rt_antialias_row_bands",
     lambda e: aab(e, e.P, f64=True, fstride=ROW32 - 8, bands=(H, 8, 8, 1)), INVALID, "f64 stride 760 < 768"),
    ("aab-first-row", "rt_antialias_row_bands", lambda e: aab(e, e.P, bands=(H, 8, 8, 1)), INVALID, "first row 13 >= height 13"),
    ("aab-pitch", "rt_antialias_row_bands", lambda e: aab(e, e.P, bands=(0, 8, 4, 2)), INVALID, "band pitch 4 < band rows 8"),
    ("edges-null-src", "rt_antialias_edges", lambda e: (e.E, None, ROW4, 0.01, e.B, ROW4, None, None), INVALID, NULL),
    ("edges-null-overlay", "rt_antialias_edges", lambda e: (e.P, e.B, ROW4, 0.01, None, ROW4, None, None), INVALID, NULL),
    ("edges-no-upload-before-nan", "rt_antialias_edges", lambda e: (e.E, e.B, ROW4, NAN, e.B, ROW4, None, None), INVALID, NO_SCENE),
    ("edges-nan-before-stride", "rt_antialias_edges", lambda e: (e.S, e.B, ROW4 - 4, NAN, e.B, ROW4, None, None), INVALID,
     "threshold is NaN"),
    ("edges-source-stride", "rt_antialias_edges", lambda e: (e.P, e.B, ROW4 - 4, 0.01, e.B, ROW4 - 4, None, None), INVALID,
     "source stride 92 < 96"),
    ("edges-overlay-stride", "rt_antialias_edges", lambda e: (e.S, e.B, ROW4, 0.01, e.B, ROW4 - 4, ctypes.byref(e.u32), None),
     INVALID, "overlay stride 92 < 96"),
    # ------------------------------------------------------------ orthogonal views
    ("ortho-null-outputs", "rt_render_ortho", lambda e: ortho(e, e.E, u8=False), INVALID, NULL),
    ("ortho-no-upload-before-axes", "rt_render_ortho", lambda e: ortho(e, e.E, a1=3), INVALID, NO_SCENE),
    ("ortho-axis-high", "rt_render_ortho", lambda e: ortho(e, e.P, a1=3), INVALID, "Invalid axes"),
    ("ortho-axis-negative", "rt_render_ortho", lambda e: ortho(e, e.S, a2=-1), INVALID, "Invalid axes"),
    ("ortho-axes-before-range", "rt_render_ortho", lambda e: ortho(e, e.P, a1=0, a2=3, y0=5, y1=3), INVALID, "Invalid axes"),
    ("ortho-range-reversed", "rt_render_ortho", lambda e: ortho(e, e.P, y0=5, y1=3), INVALID, "bad row range [5, 3)"),
    ("ortho-range-past-frame", "rt_render_ortho", lambda e: ortho(e, e.P, y1=H + 1, stride=0), INVALID, "bad row range [0, 14)"),
    ("ortho-empty-before-stride", "rt_render_ortho", lambda e: ortho(e, e.P, y0=4, y1=4, stride=0), OK, None),
    ("ortho-row-stride", "rt_render_ortho", lambda e: ortho(e, e.P, stride=ROW4 - 4, f64=True, fstride=0), INVALID,
     "row stride 92 < 96"),
    ("ortho-f64-stride", "rt_render_ortho", lambda e: ortho(e, e.P, f64=True, fstride=ROW32 - 8), INVALID, "f64 stride 760 < 768"),
    # ------------------------------------------------------------ frame assembly (no context)
    ("asm-null", "rt_assemble_row_bands", lambda e: asm(e, g=False, world=0), INVALID, NULL),
    ("asm-world", "rt_assemble_row_bands", lambda e: asm(e, world=0, height=0), INVALID, "world and band_rows must be > 0"),
    ("asm-band", "rt_assemble_row_bands", lambda e: asm(e, band=0), INVALID, "world and band_rows must be > 0"),
    ("asm-empty-before-slot", "rt_assemble_row_bands", lambda e: asm(e, height=0, slot=0), OK, None),
    ("asm-empty-row", "rt_assemble_row_bands", lambda e: asm(e, row=0, slot=0), OK, None),
    ("asm-rows-before-slot", "rt_assemble_row_bands", lambda e: asm(e, height=(1 << 24) + 1, slot=0), INVALID, "too many rows"),
    ("asm-short-slot", "rt_assemble_row_bands", lambda e: asm(e, slot=6), INVALID,
     "slot of 6 rows holds fewer than 4 bands of 2 rows"),
    ("asm-short-slot-before-stride", "rt_assemble_row_bands", lambda e: asm(e, slot=7, gstride=0), INVALID,
     "slot of 7 rows holds fewer than 4 bands of 2 rows"),
    ("asm-slot-large", "rt_assemble_row_bands", lambda e: asm(e, slot=(1 << 24) + 1, fstride=0), INVALID, "slot too large"),
    ("asm-slots-large", "rt_assemble_row_bands", lambda e: asm(e, slot=1 << 24, world=65), INVALID, "slot too large"),
    ("asm-gathered-stride", "rt_assemble_row_bands", lambda e: asm(e, gstride=ROW4 - 1), INVALID, "row stride < row bytes"),
    ("asm-frame-stride", "rt_assemble_row_bands", lambda e: asm(e, fstride=ROW4 - 1), INVALID, "row stride < row bytes"),
    ("asm-host-pointers", "rt_assemble_row_bands", lambda e: asm(e), INVALID, "frame assembly takes device pointers"),
    ("asm3-null", "rt_assemble_row_bands_rgb8", lambda e: asm(e, g=False, band=0, row=W), INVALID, NULL),
    ("asm3-world", "rt_assemble_row_bands_rgb8", lambda e: asm(e, world=0, row=0), INVALID, "world and band_rows must be > 0"),
    ("asm3-empty-before-slot", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=0, slot=0), OK, None),
    ("asm3-height-before-slot", "rt_assemble_row_bands_rgb8", lambda e: asm(e, height=(1 << 24) + 1, slot=0, row=W), INVALID,
     "frame too large"),
    ("asm3-width", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=(1 << 24) + 1), INVALID, "frame too large"),
    ("asm3-short-slot", "rt_assemble_row_bands_rgb8", lambda e: asm(e, slot=6, row=W, gstride=0), INVALID,
     "slot of 6 rows holds fewer than 4 bands of 2 rows"),
    ("asm3-slot-large", "rt_assemble_row_bands_rgb8", lambda e: asm(e, slot=(1 << 24) + 1, row=W, gstride=0), INVALID,
     "slot too large"),
    ("asm3-gathered-stride", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=W, gstride=W * 3 - 1, f=1), INVALID,
     "row stride < row bytes"),
    ("asm3-frame-stride-before-alignment", "rt_assemble_row_bands_rgb8",
     lambda e: asm(e, row=W, gstride=W * 3, fstride=ROW4 - 2), INVALID, "row stride < row bytes"),
    ("asm3-misaligned-frame", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=W, gstride=W * 3, f=1), INVALID,
     "frame rows must be 4-byte aligned"),
    ("asm3-misaligned-stride", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=W, gstride=W * 3, fstride=ROW4 + 2), INVALID,
     "frame rows must be 4-byte aligned"),
    ("asm3-host-pointers", "rt_assemble_row_bands_rgb8", lambda e: asm(e, row=W, gstride=W * 3), INVALID,
     "frame assembly takes device pointers"),
]


def test_ids_are_unique_and_every_entry_is_covered():
    assert len({r[0] for r in ROWS}) == len(ROWS)
    assert {r[1] for r in ROWS} == {
        "rt_render_points_f64", "rt_trace_pixel_f64", "rt_first_hits", "rt_first_hits_row_bands", "rt_first_hits_points",
        "rt_count_rays", "rt_count_rays_row_bands", "rt_ray_paths_offsets", "rt_ray_paths", "rt_record_rays", "rt_antialias",
        "rt_antialias_row_bands", "rt_antialias_edges", "rt_render_ortho", "rt_assemble_row_bands",
        "rt_assemble_row_bands_rgb8"}


@pytest.mark.parametrize("entry,args,status,text", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusal(env, entry, args, status, text):
    rc = getattr(env.lib, entry)(*args(env))
    got = env.lib.rt_last_error().decode()
    print(entry, rc, repr(got))
    assert rc == status
    if text is not None:
        assert got == text
    assert (env.buf == 0xA5).all() and env.n32.value == -7 and env.n64.value == 7 and env.u32.value == 7
