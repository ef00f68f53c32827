"""The two-eye cameras' host side (rt_scene_set_camera_kind / _get_camera_kind / _get_camera_eye,
include/rt_abi.h; StereoscopicCamera / AnaglyphCamera, camera.rs:82-205): no GPU needed."""
import ctypes

import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.stereo_refs import eye_centres, eye_oracle, eye_text

KINDS = ["stereoscopic", "anaglyph"]


@pytest.fixture(scope="module")
def T():
    import tinyraytracerinrust_amd as T
    return T


def compile_scene(T, text, W, H, t=0.0):
    from tinyraytracerinrust_amd.raytracer import Scene
    return Scene.compile(text, t, W, H, asset_dir=SCENES)


def bits(v):
    return np.asarray(v, np.float64).tobytes()


def test_kind_round_trip_and_default(T):
    s = compile_scene(T, scene_text("globes"), 64, 48)
    assert s.camera_kind() == ("perspective", 0.0)
    for kind, d in (("stereoscopic", 6.5), ("anaglyph", 1.0 / 3.0), ("anaglyph", -2.0), ("perspective", 0.0)):
        s.set_camera_kind(kind, d)
        assert s.camera_kind() == (kind, d)
    assert "camera" not in s.describe()
    s.set_camera_kind("anaglyph", 6.5)
    assert [l for l in s.describe().splitlines() if l.startswith("camera anaglyph eye_distance=6.5 ")]


def test_invalid_arguments(T):
    from tinyraytracerinrust_amd import _lib
    from tinyraytracerinrust_amd.raytracer import Scene
    L = _lib.lib()
    s = compile_scene(T, scene_text("globes"), 64, 48)
    out = (ctypes.c_double * 13)()
    assert L.rt_scene_set_camera_kind(s.h, 3, 1.0) == -1                 # unknown kind
    assert L.rt_scene_set_camera_kind(s.h, -1, 1.0) == -1
    for bad in (float("nan"), float("inf"), float("-inf")):               # non-finite eye distance
        assert L.rt_scene_set_camera_kind(s.h, _lib.RT_CAMERA_ANAGLYPH, bad) == -1
    assert s.camera_kind() == ("perspective", 0.0)                        # a refused call changes nothing
    assert L.rt_scene_get_camera_eye(s.h, 0, out) == -1                   # a perspective scene has no eyes
    s.set_camera_kind("anaglyph", 6.5)
    assert L.rt_scene_get_camera_eye(s.h, 2, out) == -1                   # eye index outside 0..1
    assert L.rt_scene_get_camera_eye(s.h, -1, out) == -1
    assert L.rt_scene_get_camera_eye(s.h, 1, out) == 0
    narrow = Scene.new_default(1, 8)
    assert L.rt_scene_set_camera_kind(narrow.h, _lib.RT_CAMERA_STEREOSCOPIC, 6.5) == -1   # width < 2
    assert L.rt_scene_set_camera_kind(narrow.h, _lib.RT_CAMERA_ANAGLYPH, 6.5) == 0
    with pytest.raises(ValueError):
        s.set_camera_kind("fisheye", 1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", [(64, 48), (37, 20)])
@pytest.mark.parametrize("eye_distance", [6.5, 1.0 / 3.0])
def test_eye_cameras(T, worldmap, kind, W, H, eye_distance):
    text = scene_text("globes")
    s = compile_scene(T, text, W, H)
    s.set_camera_kind(kind, eye_distance)
    centres = eye_centres(text, 0.0, eye_distance)
    # the numpy expressions on the library's own camera give the same eyes
    cam = s.camera()
    C, R = np.array(cam["center"]), np.array(cam["right"])
    h = np.float64(eye_distance) / np.float64(2.0)
    assert bits(C - R * h) == bits(centres[0]) and bits(C + R * h) == bits(centres[1])
    w = W // 2 if kind == "stereoscopic" else W
    for i in (0, 1):
        eye = s.camera_eye(i)
        assert bits(eye["center"]) == bits(centres[i])
        # the eye scene compiled at the eye camera's width: PerspectiveCamera::new(w, H, eye, ...)
        ref = compile_scene(T, eye_text(text, centres[i]), w, H).camera()
        for k in ("center", "direction", "right", "up"):
            assert bits(eye[k]) == bits(ref[k]), (i, k)
        assert bits(eye["aspect"]) == bits(ref["aspect"])
        oc = eye_oracle(text, 0.0, w, H, centres[i]).camera()
        assert bits(eye["center"]) == bits(oc[0:3]) and bits(eye["direction"]) == bits(oc[3:6])
        assert bits(eye["right"]) == bits(oc[6:9]) and bits(eye["aspect"]) == bits(oc[9])


def test_set_camera_keeps_the_kind_and_moves_the_eyes(T):
    from tinyraytracerinrust_amd import _lib
    s = compile_scene(T, scene_text("globes"), 64, 48)
    s.set_camera_kind("stereoscopic", 6.5)
    before = [s.camera_eye(i)["center"] for i in (0, 1)]
    _lib.check(_lib.lib().rt_scene_set_camera(s.h, _lib.d3((5.0, 20.0, -60.0))))
    assert s.camera_kind() == ("stereoscopic", 6.5)
    cam = s.camera()
    C, R = np.array(cam["center"]), np.array(cam["right"])
    assert list(C) == [5.0, 20.0, -60.0]
    for i, sign in ((0, -1.0), (1, 1.0)):
        eye = s.camera_eye(i)["center"]
        assert eye != before[i]
        assert bits(eye) == bits(C + sign * (R * 3.25))


def test_back_to_perspective_is_the_same_program(T):
    text = scene_text("globes")
    plain = compile_scene(T, text, 64, 48).spec_program()
    s = compile_scene(T, text, 64, 48)
    s.set_camera_kind("anaglyph", 6.5)
    two = s.spec_program()
    assert "rt_spec_views_" in two and "rt_spec_rows_" not in two and "rt_spec_prim_" not in two
    assert "rt_spec_views_" not in plain
    s.set_camera_kind("perspective", 0.0)
    assert s.spec_program() == plain


def test_tile_masks_unsupported_on_a_two_eye_scene(T):
    s = compile_scene(T, scene_text("globes"), 64, 48)
    assert s.tile_masks()[0].shape[0] == 8 * 6
    s.set_camera_kind("anaglyph", 6.5)
    with pytest.raises(T.RtError) as e:
        s.tile_masks()
    assert e.value.status == -6 and "two-eye" in e.value.message


def test_cli_camera_options():
    from tinyraytracerinrust_amd.__main__ import _parse
    a = _parse(["render", "x.scene", "--camera", "anaglyph", "--eye-distance", "6.5"])
    assert (a.camera, a.eye_distance) == ("anaglyph", 6.5)
    a = _parse(["render", "x.scene", "--camera", "stereoscopic", "--eye-distance", "0.25", "--gpus", "2"])
    assert (a.camera, a.eye_distance, a.gpus) == ("stereoscopic", 0.25, 2)
    assert _parse(["render", "x.scene"]).camera == "perspective"
    for kind in KINDS:
        with pytest.raises(SystemExit):
            _parse(["render", "x.scene", "--camera", kind])
    with pytest.raises(SystemExit):
        _parse(["render", "x.scene", "--camera", "fisheye", "--eye-distance", "1"])
