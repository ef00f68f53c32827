"""First-hit maps (rt_first_hits, rt_first_hits_row_bands, rt_first_hits_points) without a GPU: the library exports
and the binding declares the three entry points, the plane struct has the ABI's layout, a NULL context is refused,
and the headless driver's parser takes the four map flags as documented."""
import ctypes

import pytest

NAMES = ("rt_first_hits", "rt_first_hits_row_bands", "rt_first_hits_points")
FLAGS = ("--object-map", "--depth-map", "--normal-map", "--shadow-map")
RT_ERR_INVALID = -1


def test_library_exports_the_three_symbols():
    import tinyraytracerinrust_amd as T
    lib = T.lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_binding_declares_the_three_symbols():
    from tinyraytracerinrust_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
    # rt_first_hits(ctx, y0, y1, planes, stream); the band form takes four geometry words;
    # rt_first_hits_points(ctx, xy, n, object, distance, shadow, normal, stream)
    assert len(_lib.SIGNATURES["rt_first_hits"][1]) == 5
    assert len(_lib.SIGNATURES["rt_first_hits_row_bands"][1]) == 7
    assert len(_lib.SIGNATURES["rt_first_hits_points"][1]) == 8


def test_hit_planes_struct_is_four_pointer_stride_pairs():
    from tinyraytracerinrust_amd import _lib
    assert ctypes.sizeof(_lib.rt_hit_planes) == 64
    assert [f[0] for f in _lib.rt_hit_planes._fields_] == [
        "object", "object_stride", "distance", "distance_stride", "shadow", "shadow_stride", "normal", "normal_stride"]
    assert [getattr(_lib.rt_hit_planes, f[0]).offset for f in _lib.rt_hit_planes._fields_] == list(range(0, 64, 8))


def test_null_context_is_refused():
    import tinyraytracerinrust_amd as T
    lib = T.lib()
    obj = (ctypes.c_int32 * 4)()
    planes = T._lib.rt_hit_planes(object=ctypes.addressof(obj), object_stride=16)
    xy = (ctypes.c_double * 2)(0.0, 0.0)
    assert lib.rt_first_hits(None, 0, 1, ctypes.byref(planes), None) == RT_ERR_INVALID
    assert lib.rt_first_hits_row_bands(None, 0, 1, 1, 1, ctypes.byref(planes), None) == RT_ERR_INVALID
    assert lib.rt_first_hits_points(None, ctypes.addressof(xy), 1, ctypes.addressof(obj), None, None, None,
                                    None) == RT_ERR_INVALID
    assert list(obj) == [0, 0, 0, 0]


@pytest.mark.parametrize("flag", FLAGS)
def test_parser_accepts_each_map_flag(flag):
    from tinyraytracerinrust_amd.__main__ import _parse
    a = _parse(["render", "x.scene", flag, "m.png"])
    dest = flag[2:].replace("-", "_")
    assert getattr(a, dest) == "m.png"
    assert [getattr(a, f[2:].replace("-", "_")) for f in FLAGS if f != flag] == [None] * 3
    a = _parse(["render", "x.scene", flag, "m.png", "--camera", "stereoscopic", "--eye-distance", "6.5"])
    assert getattr(a, dest) == "m.png" and a.camera == "stereoscopic"


def test_parser_accepts_the_four_flags_together():
    from tinyraytracerinrust_amd.__main__ import _parse
    a = _parse(["render", "x.scene", "--object-map", "o.png", "--depth-map", "d.png", "--normal-map", "n.png",
                "--shadow-map", "s.png"])
    assert (a.object_map, a.depth_map, a.normal_map, a.shadow_map) == ("o.png", "d.png", "n.png", "s.png")
    b = _parse(["render", "x.scene"])
    assert (b.object_map, b.depth_map, b.normal_map, b.shadow_map) == (None,) * 4


@pytest.mark.parametrize("flag", FLAGS)
def test_parser_refuses_a_map_with_several_gpus(flag, capsys):
    from tinyraytracerinrust_amd.__main__ import _parse
    with pytest.raises(SystemExit) as e:
        _parse(["render", "x.scene", flag, "m.png", "--gpus", "2"])
    assert e.value.code != 0
    assert flag in capsys.readouterr().err


@pytest.mark.parametrize("flag", FLAGS)
def test_parser_refuses_a_map_of_an_anaglyph_scene(flag, capsys):
    from tinyraytracerinrust_amd.__main__ import _parse
    with pytest.raises(SystemExit) as e:
        _parse(["render", "x.scene", flag, "m.png", "--camera", "anaglyph", "--eye-distance", "6.5"])
    assert e.value.code != 0
    assert flag in capsys.readouterr().err


def test_hit_maps_of_host_planes():
    """The maps' arithmetic on a hand-made 1x4 frame: a miss, the nearest and the farthest hit, a shadowed hit."""
    import argparse
    import numpy as np
    from tinyraytracerinrust_amd.__main__ import hit_maps
    a = argparse.Namespace(object_map="o", depth_map="d", normal_map="n", shadow_map="s")
    planes = {"object": np.array([[-1, 0, 5, 2]], np.int32),
              "distance": np.array([[np.inf, 10.0, 30.0, 20.0]]),
              "shadow": np.array([[0, 0, 3, 1]], np.uint32),
              "normal": np.array([[[0, 0, 0], [0, 0, -2.0], [3.0, 0, 0], [0, 0.5, 0]]])}
    maps = dict(hit_maps(a, planes, 6, 2))
    assert maps["o"].tolist() == [[0, 42, 255, 127]]            # (1 + o) * 255 // 6
    assert maps["d"].tolist() == [[0, 255, 64, 159]]            # white .. dark grey, linear
    assert maps["s"].tolist() == [[0, 255, 0, 127]]             # lights seen / lights
    assert maps["n"][0, :, :3].tolist() == [[0, 0, 0], [127, 127, 0], [255, 127, 127], [127, 255, 127]]
    assert all(m.dtype == np.uint8 for m in maps.values())
