"""Reference frames for the two-eye cameras (camera.rs:82-205), composed from the CPU oracle.

An eye is a plain PerspectiveCamera at a shifted centre, so the oracle renders it when the scene text
places its camera there: ``set camera(<x, y, z>)`` appended at top level (where the DSL's camera
transform is the identity), each coordinate written as its exact decimal expansion (the DSL's number
literal has no exponent form; its parser is correctly rounded).  The helper asserts that the oracle's
camera centre comes back bitwise equal to the numpy value.
"""
import functools
import math
from decimal import Decimal

import numpy as np

from tests.conftest import scene_text

EYE_DISTANCE = 6.5


def exact_decimal(v: float) -> str:
    s = format(Decimal(abs(float(v))), "f")
    return ("-" if math.copysign(1.0, v) < 0 else "") + s


def eye_centres(text: str, time: float, eye_distance: float):
    """(left_eye, right_eye) in numpy f64 from the oracle's own camera: C -+ R * (eye_distance / 2.0),
    one multiply then one subtract / add per component (camera.rs:108-109)."""
    from oracle import oracle as O
    cam = O.OracleScene(text, time, 16, 16).camera()     # centre and right do not depend on the frame size
    C, R = cam[0:3].astype(np.float64), cam[6:9].astype(np.float64)
    h = np.float64(eye_distance) / np.float64(2.0)
    return C - R * h, C + R * h


def eye_text(text: str, centre) -> str:
    return text.rstrip("\n") + "\nset camera(<" + ", ".join(exact_decimal(v) for v in centre) + ">)\n"


def eye_oracle(text: str, time: float, width: int, height: int, centre, max_depth: int = 10):
    """The oracle scene of one eye at width x height; its camera centre is bitwise `centre`."""
    from oracle import oracle as O
    sc = O.OracleScene(eye_text(text, centre), time, width, height, max_depth=max_depth)
    assert sc.status == 0, sc.error
    got = sc.camera()[0:3]
    assert got.tobytes() == np.asarray(centre, np.float64).tobytes(), (got, centre)
    return sc


def quantise(c: np.ndarray) -> np.ndarray:
    """`(c * 255.0) as u8` (easy_pixbuf.rs:49-52): truncation, saturating, NaN -> 0."""
    v = np.nan_to_num(np.asarray(c, np.float64) * 255.0, nan=0.0, posinf=255.0, neginf=0.0)
    return np.trunc(np.clip(v, 0.0, 255.0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name: str, time: float, W: int, H: int, depth: int, kind: str, eye_distance: float = EYE_DISTANCE):
    """(f64 (H, W, 4), u8 (H, W, 4)) of the whole frame; computed once per case, never modified."""
    text = scene_text(name)
    left, right = eye_centres(text, time, eye_distance)
    if kind == "anaglyph":
        Lf, Lu = eye_oracle(text, time, W, H, left, depth).render(f64=True)
        Rf, Ru = eye_oracle(text, time, W, H, right, depth).render(f64=True)
        f = Rf.copy(); f[..., 0] = Lf[..., 0]; f[..., 3] = 1.0
        u = Ru.copy(); u[..., 0] = Lu[..., 0]; u[..., 3] = 255
    else:
        assert kind == "stereoscopic"
        w = W // 2
        Ls, Rs = eye_oracle(text, time, w, H, left, depth), eye_oracle(text, time, w, H, right, depth)
        Lf, Lu = Ls.render(f64=True)
        Rf, Ru = Rs.render(f64=True)
        f, u = np.zeros((H, W, 4)), np.zeros((H, W, 4), np.uint8)
        f[:, :w], u[:, :w] = Rf, Ru                       # x < w: the RIGHT camera at (x, y)
        f[:, w:2 * w], u[:, w:2 * w] = Lf, Lu             # x >= w: the LEFT camera at (x - w, y)
        if W % 2:                                         # odd W: the left camera at x - w = w
            for y in range(H):
                f[y, W - 1] = Ls.get_pixel(float(w), float(y))
            u[:, W - 1] = quantise(f[:, W - 1])
            u[:, W - 1, 3] = 255
    f.setflags(write=False)
    u.setflags(write=False)
    return f, u


def point_reference(name: str, time: float, W: int, H: int, depth: int, kind: str, xy, eye_distance: float = EYE_DISTANCE):
    """get_pixel(x, y) of the two-eye camera at each (x, y), composed from the oracle's get_pixel."""
    text = scene_text(name)
    left, right = eye_centres(text, time, eye_distance)
    w = W // 2 if kind == "stereoscopic" else W
    Ls, Rs = eye_oracle(text, time, w, H, left, depth), eye_oracle(text, time, w, H, right, depth)
    out = []
    for x, y in xy:
        if kind == "stereoscopic":
            out.append(Ls.get_pixel(x - float(w), y) if x >= float(w) else Rs.get_pixel(x, y))
        else:
            l, r = Ls.get_pixel(x, y), Rs.get_pixel(x, y)
            out.append(np.array([l[0], r[1], r[2], 1.0]))
    return np.array(out)
