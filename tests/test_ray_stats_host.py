"""Ray counts (rt_count_rays, rt_count_rays_row_bands) without a GPU: the library exports and the binding declares
both entry points, the result struct has the ABI's size, and the headless driver's parser takes --count-rays and
--ray-map as documented."""
import ctypes

import pytest

NAMES = ("rt_count_rays", "rt_count_rays_row_bands")


def test_library_exports_both_symbols():
    import tinyraytracerinrust_amd as T
    lib = T.lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_binding_declares_both_symbols():
    from tinyraytracerinrust_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
    # rt_count_rays(ctx, y0, y1, depth, totals, rows, pixels, stride, stream); the band form takes four geometry words
    assert len(_lib.SIGNATURES["rt_count_rays"][1]) == 9
    assert len(_lib.SIGNATURES["rt_count_rays_row_bands"][1]) == 11


def test_ray_counts_struct_is_four_u64():
    from tinyraytracerinrust_amd import _lib
    assert ctypes.sizeof(_lib.rt_ray_counts) == 32
    assert [f[0] for f in _lib.rt_ray_counts._fields_] == ["primary", "shadow", "reflect", "refract"]


def test_null_context_is_refused():
    import tinyraytracerinrust_amd as T
    t = T._lib.rt_ray_counts()
    assert T.lib().rt_count_rays(None, 0, 1, -1, ctypes.byref(t), None, None, 0, None) == -1          # RT_ERR_INVALID
    assert T.lib().rt_count_rays_row_bands(None, 0, 1, 1, 1, -1, ctypes.byref(t), None, None, 0, None) == -1


def test_parser_rejects_ray_map_with_several_gpus(capsys):
    from tinyraytracerinrust_amd.__main__ import _parse
    with pytest.raises(SystemExit) as e:
        _parse(["render", "x.scene", "--ray-map", "x.png", "--gpus", "2"])
    assert e.value.code != 0
    assert "--ray-map" in capsys.readouterr().err


def test_parser_accepts_ray_map_and_count_rays():
    from tinyraytracerinrust_amd.__main__ import _parse
    a = _parse(["render", "x.scene", "--ray-map", "x.png"])
    assert a.ray_map == "x.png" and a.count_rays                  # the map implies the count
    a = _parse(["render", "x.scene", "--count-rays", "--camera", "anaglyph", "--eye-distance", "6.5"])
    assert a.count_rays and a.ray_map is None and a.camera == "anaglyph" and a.eye_distance == 6.5
    a = _parse(["render", "x.scene", "--count-rays", "--gpus", "2"])
    assert a.count_rays and a.gpus == 2
    assert not _parse(["render", "x.scene"]).count_rays
