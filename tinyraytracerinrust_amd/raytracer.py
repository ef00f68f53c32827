"""Host-side mirror of the reference's render-path interface, over the C ABI.

Mirrors the names and argument meaning of the reference (andreivasiliu/TinyRaytracerInRust):

* ``MatrixTransformation`` / ``TransformationStack``  -- src/raytracer/transformation.rs:7-205
* ``RayTracer``  -- src/raytracer/raytracer.rs:21-364 (new_default, add_test_objects, add_object,
  add_light, set_camera_from_vector, get_pixel, max_depth) plus the DebugWindow row loop
  ``render_lines`` (src/raydebugger/debug_window.rs:74-87) and ``load_scene``
  (src/sceneparser/scene_loader.rs:24-47, as reached from debug_window.rs:53-62).

Everything renders on the GPU through librt_mi355x.so; there is no CPU path.  Device buffers are
torch tensors (``torch`` is plumbing for HBM allocations and streams), host results are numpy.
"""
from __future__ import annotations

import ctypes
import os
import sys as _sys
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import check, d3, d4, lib

MAX_FRAMES = 300   # src/raydebugger/gui.rs:20 -- the GUI's time = frame / MAX_FRAMES


class MatrixTransformation:
    """transformation.rs:47-205: a 4x4 matrix and its separately built inverse."""

    def __init__(self, xf: Optional[_lib.rt_transformation] = None):
        self.xf = xf if xf is not None else _lib.rt_transformation()
        if xf is None:
            check(lib().rt_xform_identity(ctypes.byref(self.xf)))

    @classmethod
    def create_identity_matrix(cls) -> "MatrixTransformation":
        return cls()

    @classmethod
    def _make(cls, fn, x, y, z) -> "MatrixTransformation":
        t = _lib.rt_transformation()
        check(fn(float(x), float(y), float(z), ctypes.byref(t)))
        return cls(t)

    @classmethod
    def create_translation_matrix(cls, x, y, z):
        return cls._make(lib().rt_xform_translation, x, y, z)

    @classmethod
    def create_rotation_matrix(cls, x, y, z):
        return cls._make(lib().rt_xform_rotation, x, y, z)

    @classmethod
    def create_scaling_matrix(cls, x, y, z):
        return cls._make(lib().rt_xform_scaling, x, y, z)

    def compose_with(self, other: "MatrixTransformation") -> "MatrixTransformation":
        out = _lib.rt_transformation()
        check(lib().rt_xform_compose(ctypes.byref(self.xf), ctypes.byref(other.xf), ctypes.byref(out)))
        return MatrixTransformation(out)

    @property
    def matrix(self) -> np.ndarray:
        return np.array(self.xf.matrix[:]).reshape(4, 4)

    @property
    def inverse_matrix(self) -> np.ndarray:
        return np.array(self.xf.inverse[:]).reshape(4, 4)

    def transform_vector(self, v: Sequence[float]) -> np.ndarray:
        """transformation.rs:53-59, left-to-right sums."""
        m = self.xf.matrix
        x, y, z = (float(c) for c in v)
        return np.array([m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3] for r in range(3)])


class TransformationStack:
    """transformation.rs:7-37."""

    def __init__(self):
        self.stack = [MatrixTransformation.create_identity_matrix()]

    def push_transformation(self, t: MatrixTransformation) -> None:
        self.stack.append(t.compose_with(self.stack[-1]) if self.stack else t)

    def pop_transformation(self) -> MatrixTransformation:
        if not self.stack:
            raise IndexError("Trying to pop from an empty TransformationStack!")
        return self.stack.pop()

    def get_transformation(self) -> MatrixTransformation:
        return self.stack[-1]


def solid_material(color=(0.0, 0.0, 0.0, 1.0), reflectivity=0.0, transparency=0.0) -> _lib.rt_material:
    """SolidColorMaterial::new (material.rs:41-49); RTObject::new's default is BLACK (rt_object.rs:13-20)."""
    c = list(color) + [1.0] * (4 - len(color))
    return _lib.rt_material(d4(c), -1, float(reflectivity), float(transparency))


def textured_material(texture_id: int, reflectivity=0.0, transparency=0.0) -> _lib.rt_material:
    """TexturedMaterial::new (material.rs:76-84)."""
    return _lib.rt_material(d4((0, 0, 0, 1)), int(texture_id), float(reflectivity), float(transparency))


class Scene:
    """Owner of an ``rt_scene*`` (the RayTracer's scene content)."""

    def __init__(self, handle: int, width: int, height: int, status: int = 0, error: str = ""):
        self.h = ctypes.c_void_p(handle)
        self.width, self.height = width, height
        self.status, self.error = status, error

    @classmethod
    def new_default(cls, width: int, height: int) -> "Scene":
        h = ctypes.c_void_p()
        check(lib().rt_scene_new(width, height, ctypes.byref(h)))
        return cls(h.value, width, height)

    @classmethod
    def compile(cls, text: str, time: float, width: int, height: int,
                asset_dir: Optional[str] = None, strict: bool = True) -> "Scene":
        """load_scene on a fresh new_default()+add_test_objects() RayTracer.

        A parse error raises when ``strict``; otherwise the default scene is returned with
        ``status``/``error`` set, as the reference prints the error and renders on
        (debug_window.rs:58-60)."""
        h = ctypes.c_void_p()
        rc = lib().rt_scene_compile(text.encode(), asset_dir.encode() if asset_dir else None,
                                    float(time), width, height, ctypes.byref(h))
        if rc == -2 and not strict and h.value:
            return cls(h.value, width, height, rc, lib().rt_last_error().decode())
        check(rc)
        return cls(h.value, width, height)

    def info(self) -> dict:
        no, nl, nlf = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().rt_scene_info(self.h, ctypes.byref(no), ctypes.byref(nl), ctypes.byref(nlf),
                                  ctypes.byref(w), ctypes.byref(h)))
        return {"objects": no.value, "lights": nl.value, "leaves": nlf.value,
                "width": w.value, "height": h.value}

    def trace_pixel(self, x: float, y: float, max_depth: int = -1, device: int = 0) -> np.ndarray:
        """rt_trace_pixel_f64: RayTracer::get_pixel(x, y) of this scene, traced on GPU ``device``
        (no context of the caller's; one upload per call).  Returns 4 doubles (r, g, b, a)."""
        out = np.empty(4, np.float64)
        check(lib().rt_trace_pixel_f64(self.h, float(x), float(y), int(max_depth), int(device),
                                       ctypes.c_void_p(out.ctypes.data)))
        return out

    def traversal(self) -> List[Tuple[int, int]]:
        """The kernels' object hierarchy: pre-order (obj, skip) nodes, obj = -1 for a group."""
        n = ctypes.c_int32()
        check(lib().rt_scene_traversal(self.h, None, None, 0, ctypes.byref(n)))
        obj, skip = (ctypes.c_int32 * max(1, n.value))(), (ctypes.c_int32 * max(1, n.value))()
        check(lib().rt_scene_traversal(self.h, obj, skip, n.value, ctypes.byref(n)))
        return [(obj[i], skip[i]) for i in range(n.value)]

    def describe(self) -> str:
        """rt_scene_describe: the flattened scene (flags, hierarchies, culling records) as text."""
        n = ctypes.c_size_t()
        check(lib().rt_scene_describe(self.h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        check(lib().rt_scene_describe(self.h, buf, n.value + 1, ctypes.byref(n)))
        return buf.value.decode()

    def spec_program(self) -> str:
        """rt_scene_spec_program: the scene-specialised program's text (RT_OPT_SPECIALIZE)."""
        n = ctypes.c_size_t()
        check(lib().rt_scene_spec_program(self.h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        check(lib().rt_scene_spec_program(self.h, buf, n.value + 1, ctypes.byref(n)))
        return buf.value.decode()

    def tile_masks(self, y_first: int = 0, band_rows: Optional[int] = None, band_pitch: Optional[int] = None,
                   n_bands: int = 1):
        """rt_scene_tile_masks: the per-tile object masks of a band launch (default: the whole frame),
        evaluated on the host -> (uint32 array [tiles, 6]: prim, shadow[0..3], refl; info dict)."""
        band_rows = self.height - y_first if band_rows is None else band_rows
        band_pitch = band_rows if band_pitch is None else band_pitch
        tiles = ((self.width + 7) // 8) * ((band_rows * n_bands + 7) // 8)
        words = np.zeros((tiles, _lib.RT_TILEMASK_WORDS), dtype=np.uint32)
        info = (ctypes.c_int32 * 4)()
        check(lib().rt_scene_tile_masks(self.h, y_first, band_rows, band_pitch, n_bands,
                                        ctypes.c_void_p(words.ctypes.data), words.size, info))
        assert info[0] == tiles, (info[0], tiles)
        return words, {"tiles": info[0], "plane": info[1], "boxed": info[2] & 0xffffffff, "valid": bool(info[3])}

    def precompile(self) -> float:
        """rt_scene_precompile: compile the specialised program into the process cache (no device);
        returns the hipRTC milliseconds (0 when cached)."""
        ms = ctypes.c_double()
        check(lib().rt_scene_precompile(self.h, ctypes.byref(ms)))
        return ms.value

    def spec_report(self) -> str:
        """rt_scene_spec_report: compile (or find) the scene's specialised programs and describe them --
        the compiler, and per kernel its VGPRs, spills, scratch, occupancy and where it came from."""
        n = ctypes.c_size_t()
        check(lib().rt_scene_spec_report(self.h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        check(lib().rt_scene_spec_report(self.h, buf, n.value + 1, ctypes.byref(n)))
        return buf.value.decode()

    def sample_report(self) -> str:
        """rt_scene_sample_report: compile (or find) the scene's two sample programs (rt_spec_points,
        rt_spec_aa: the specialised kernels of render_points and of the anti-aliasing trace) and describe
        them, one line per kernel in spec_report's format."""
        n = ctypes.c_size_t()
        check(lib().rt_scene_sample_report(self.h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        check(lib().rt_scene_sample_report(self.h, buf, n.value + 1, ctypes.byref(n)))
        return buf.value.decode()

    def lean_report(self) -> str:
        """rt_scene_lean_report: compile (or find) the scene's lean kernels (RT_OPT_LEAN_TILES: rt_spec_lean_0 and
        rt_spec_lean_check) and describe them, one line per kernel in spec_report's format; "" for a scene whose
        programs hold none."""
        n = ctypes.c_size_t()
        check(lib().rt_scene_lean_report(self.h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        check(lib().rt_scene_lean_report(self.h, buf, n.value + 1, ctypes.byref(n)))
        return buf.value.decode()

    @staticmethod
    def register_family(scenes) -> float:
        """rt_spec_family_register: one specialised program for scenes of the same structure (the
        frames of an animation); renderers whose scene belongs to it load that program when
        specialisation is on.  Returns the hipRTC milliseconds (0 when cached)."""
        arr = (ctypes.c_void_p * len(scenes))(*[s.h.value for s in scenes])
        ms = ctypes.c_double()
        check(lib().rt_spec_family_register(arr, len(scenes), ctypes.byref(ms)))
        return ms.value

    @staticmethod
    def clear_families() -> None:
        """rt_spec_family_clear: forget every registered scene family."""
        check(lib().rt_spec_family_clear())

    def camera(self) -> dict:
        out = (ctypes.c_double * 13)()
        check(lib().rt_scene_get_camera(self.h, out))
        v = list(out)
        return {"center": v[0:3], "direction": v[3:6], "right": v[6:9], "up": v[9:12], "aspect": v[12]}

    def set_camera_kind(self, kind: str, eye_distance: float = 0.0) -> None:
        """rt_scene_set_camera_kind: "perspective", "stereoscopic" (camera.rs:82-141) or "anaglyph" (:143-205)."""
        if kind not in _lib.CAMERA_KINDS:
            raise ValueError(f"camera kind {kind!r} not in {sorted(_lib.CAMERA_KINDS)}")
        check(lib().rt_scene_set_camera_kind(self.h, _lib.CAMERA_KINDS[kind], float(eye_distance)))

    def camera_kind(self) -> Tuple[str, float]:
        """(kind, eye_distance) as set_camera_kind took them; ("perspective", 0.0) by default."""
        k, d = ctypes.c_int32(), ctypes.c_double()
        check(lib().rt_scene_get_camera_kind(self.h, ctypes.byref(k), ctypes.byref(d)))
        return {v: n for n, v in _lib.CAMERA_KINDS.items()}[k.value], d.value

    def camera_eye(self, i: int) -> dict:
        """Eye i (0 left, 1 right) of a stereoscopic / anaglyph scene, as camera()."""
        out = (ctypes.c_double * 13)()
        check(lib().rt_scene_get_camera_eye(self.h, int(i), out))
        v = list(out)
        return {"center": v[0:3], "direction": v[3:6], "right": v[6:9], "up": v[9:12], "aspect": v[12]}

    def light(self, i: int) -> Tuple[list, list]:
        p, c = (ctypes.c_double * 3)(), (ctypes.c_double * 4)()
        check(lib().rt_scene_get_light(self.h, i, p, c))
        return list(p), list(c)

    def free(self) -> None:
        if self.h and self.h.value:
            lib().rt_scene_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _check_rows(a, dtype: str, what: str) -> None:
    """The library reads and writes packed rows of one element type behind a row stride: refuse an array
    (numpy or torch) of another dtype, or whose rows are not contiguous, before its address is passed."""
    if str(a.dtype).split(".")[-1] != dtype:
        raise ValueError(f"{what} is {a.dtype}, not {dtype}")
    if a.shape[0] and not (a[0].flags.c_contiguous if isinstance(a, np.ndarray) else a[0].is_contiguous()):
        raise ValueError(f"the rows of the {what} must be contiguous")


def _address(a) -> Tuple[int, int]:
    """(address, row stride in bytes) of a numpy array or a torch tensor, as the library takes a plane."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data, a.strides[0]
    return a.data_ptr(), a.stride(0) * a.element_size()


def _stream_handle(stream, device=None) -> int:
    """The stream a call runs on, as the library takes it: ``stream`` (a torch.cuda.Stream) if given; else torch's
    current stream on ``device`` (a torch device or an index) when the call involves a device tensor; else 0, the
    device's default stream.  Imports torch only for the current stream."""
    if stream is not None:
        return stream.cuda_stream
    if device is None:
        return 0
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class Renderer:
    """Owner of an ``rt_ctx*``: one device, its stream, the uploaded scene."""

    # RT_OPT_SPECIALIZE for new renderers: None keeps the library's default (1: the scene's kernels
    # compiled in the background after each upload, taken once ready).  tests/conftest.py sets 0 so
    # that tests which pin a kernel choice see a deterministic one; the specialised paths have tests of
    # their own (tests/test_gpu_spec*.py, test_gpu_spec_async.py).
    LIBRARY_DEFAULT = -1            # specialize=LIBRARY_DEFAULT: leave the option as the library sets it
    default_specialize: Optional[int] = None

    def __init__(self, device: int = 0, specialize: Optional[int] = None):
        h = ctypes.c_void_p()
        check(lib().rt_ctx_create(int(device), ctypes.byref(h)))
        self.h = h
        Renderer._register(self)
        self.device = device
        self.width = self.height = 0
        level = specialize if specialize is not None else Renderer.default_specialize
        if level is not None and level != Renderer.LIBRARY_DEFAULT:
            self.set_specialize(level, wait=False)

    def upload(self, scene: Scene) -> None:
        check(lib().rt_ctx_upload(self.h, scene.h))
        self.width, self.height = scene.width, scene.height

    def render_rows_into(self, y0: int, y1: int, out_ptr: int, row_stride: int, max_depth: int = -1,
                         stream: Optional[int] = None, f64: bool = False) -> None:
        fn = lib().rt_render_rows_f64 if f64 else lib().rt_render_rows
        check(fn(self.h, y0, y1, max_depth, ctypes.c_void_p(out_ptr), row_stride, ctypes.c_void_p(stream or 0)))

    def render_rows(self, y0: int, y1: int, max_depth: int = -1, f64: bool = False, out=None,
                    stream=None):
        """Render rows [y0, y1) into a device tensor (torch, on this device) and return it.

        uint8 RGBA (rows, W, 4) by default, float64 RGBA with ``f64``.  Runs on ``stream``
        (a torch.cuda.Stream) or torch's current stream, asynchronously."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((y1 - y0, self.width, 4), dtype=torch.float64 if f64 else torch.uint8, device=dev)
        self.render_rows_into(y0, y1, *_address(out), max_depth, _stream_handle(stream, dev), f64)
        return out

    def rows_launcher(self, y0: int, y1: int, out, max_depth: int = -1, stream=None):
        """A zero-argument callable that launches rt_render_rows(y0, y1) into the device tensor ``out``
        on ``stream`` (torch's current stream by default) each time it is called: the arguments are
        converted once, so a host loop pays one ctypes call per frame -- what a native host's FFI call
        costs -- instead of this wrapper's per-call argument handling (a 1080p single-sphere frame takes
        ~19 us on the GPU, the same order as that handling)."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device))
        fn = lib().rt_render_rows
        args = (self.h, ctypes.c_uint32(y0), ctypes.c_uint32(y1), ctypes.c_int32(max_depth), ctypes.c_void_p(out.data_ptr()),
                ctypes.c_size_t(out.stride(0) * out.element_size()), ctypes.c_void_p(st.cuda_stream))
        keep = out

        def launch():
            rc = fn(*args)
            if rc < 0:
                check(rc)
            return keep
        return launch

    def render_row_bands(self, y_first: int, band_rows: int, band_pitch: int, n_bands: int, out,
                         max_depth: int = -1, stream=None) -> None:
        """rt_render_row_bands into a device uint8 tensor ``out`` of >= n_bands*band_rows rows: RGBA8
        (rows, W, 4), or packed RGB8 (rows, W, 3) through rt_render_row_bands_rgb8."""
        fn = lib().rt_render_row_bands_rgb8 if out.shape[-1] == 3 else lib().rt_render_row_bands
        ptr, stride = _address(out)
        check(fn(self.h, y_first, band_rows, band_pitch, n_bands, max_depth, ctypes.c_void_p(ptr), stride,
                 ctypes.c_void_p(_stream_handle(stream, self.device))))

    def render_rows_host(self, y0: int, y1: int, max_depth: int = -1, f64: bool = False) -> np.ndarray:
        """Synchronous render into a host numpy array (the library stages through HBM)."""
        out = np.empty((y1 - y0, self.width, 4), np.float64 if f64 else np.uint8)
        self.render_rows_into(y0, y1, out.ctypes.data, out.strides[0], max_depth, None, f64)
        return out

    def render_points(self, xy: np.ndarray, max_depth: int = -1) -> np.ndarray:
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((xy.shape[0], 4), np.float64)
        check(lib().rt_render_points_f64(self.h, ctypes.c_void_p(xy.ctypes.data), xy.shape[0], max_depth,
                                         ctypes.c_void_p(out.ctypes.data), None))
        return out

    def antialias(self, frame, threshold: float = 0.01, level: int = 3, max_depth: int = -1, f64: bool = False,
                  out=None, stream=None):
        """rt_antialias over a whole quantised frame.  ``frame`` is an (H, W, 4) uint8 torch tensor
        on this device (returns a device tensor; asynchronous up to the edge count) or a numpy
        array (returns numpy).  Returns (anti-aliased frame, sub-pixel rays traced); the frame is
        float64 RGBA with ``f64``."""
        rays = ctypes.c_uint64(0)
        host = isinstance(frame, np.ndarray)
        if host:
            src = np.ascontiguousarray(frame, dtype=np.uint8)
            res = out if out is not None else np.empty(src.shape, np.float64 if f64 else np.uint8)
        else:
            import torch
            src = frame
            res = out if out is not None else torch.empty(tuple(frame.shape), dtype=torch.float64 if f64 else torch.uint8,
                                                          device=frame.device)
        (sp, ss), (rp, rs) = _address(src), _address(res)
        st = 0 if host else _stream_handle(stream, frame.device)
        u8p, u8s, fp, fs = (None, 0, rp, rs) if f64 else (rp, rs, None, 0)
        check(lib().rt_antialias(self.h, ctypes.c_void_p(sp), ss, float(threshold), int(level), int(max_depth),
                                 ctypes.c_void_p(u8p), u8s, ctypes.c_void_p(fp), fs, ctypes.byref(rays),
                                 ctypes.c_void_p(st)))
        return res, rays.value

    def antialias_row_bands(self, frame, y_first: int, band_rows: int, band_pitch: int, n_bands: int,
                            threshold: float = 0.01, level: int = 3, max_depth: int = -1, f64: bool = False,
                            out=None, stream=None):
        """rt_antialias_row_bands: the anti-aliasing pass for the rows of a band layout (the geometry of
        render_row_bands).  ``frame`` is the WHOLE (H, W, 4) quantised frame, a torch tensor on this
        device or a numpy array, as for ``antialias``.  Returns (packed rows, sub-pixel rays traced in
        them): band b row j at row b*band_rows + j of an (n_bands*band_rows, W, 4) array (``out``, if
        given, needs at least that many rows); rows past the frame's height are not written."""
        rays = ctypes.c_uint64(0)
        rows = int(band_rows) * int(n_bands)
        host = isinstance(frame, np.ndarray)
        if host:
            src = np.ascontiguousarray(frame, dtype=np.uint8)
            res = out if out is not None else np.zeros((rows, src.shape[1], 4), np.float64 if f64 else np.uint8)
        else:
            import torch
            src = frame
            res = out if out is not None else torch.zeros((rows, frame.shape[1], 4),
                                                          dtype=torch.float64 if f64 else torch.uint8, device=frame.device)
        (sp, ss), (rp, rs) = _address(src), _address(res)
        st = 0 if host else _stream_handle(stream, frame.device)
        if tuple(src.shape) != (self.height, self.width, 4):
            raise ValueError(f"frame {tuple(src.shape)} is not the uploaded scene's {(self.height, self.width, 4)}")
        if res.shape[0] < rows or tuple(res.shape[1:]) != (self.width, 4):
            raise ValueError(f"output {tuple(res.shape)} holds fewer than {rows} rows of {(self.width, 4)}")
        _check_rows(src, "uint8", "frame")
        _check_rows(res, "float64" if f64 else "uint8", "output")
        if res.shape[0] == 0:                 # no band and no output row: an empty tensor has no address to pass
            return res, 0
        u8p, u8s, fp, fs = (None, 0, rp, rs) if f64 else (rp, rs, None, 0)
        check(lib().rt_antialias_row_bands(self.h, ctypes.c_void_p(sp), ss, float(threshold), int(level), int(max_depth),
                                           int(y_first), int(band_rows), int(band_pitch), int(n_bands),
                                           ctypes.c_void_p(u8p), u8s, ctypes.c_void_p(fp), fs, ctypes.byref(rays),
                                           ctypes.c_void_p(st)))
        return res, rays.value

    def antialias_edges(self, frame, threshold: float = 0.01):
        """rt_antialias_edges: the GUI's "show edges" overlay of a whole quantised frame (torch device
        tensor or numpy array, as for ``antialias``).  Returns ((H, W, 4) uint8 overlay, marked pixels)."""
        n = ctypes.c_uint32(0)
        host = isinstance(frame, np.ndarray)
        if host:
            src = np.ascontiguousarray(frame, dtype=np.uint8)
            res = np.empty(src.shape, np.uint8)
        else:
            import torch
            src = frame
            res = torch.empty(tuple(frame.shape), dtype=torch.uint8, device=frame.device)
        (sp, ss), (rp, rs) = _address(src), _address(res)
        st = 0 if host else _stream_handle(None, frame.device)
        if tuple(src.shape) != (self.height, self.width, 4):
            raise ValueError(f"frame {tuple(src.shape)} is not the uploaded scene's {(self.height, self.width, 4)}")
        _check_rows(src, "uint8", "frame")
        check(lib().rt_antialias_edges(self.h, ctypes.c_void_p(sp), ss, float(threshold), ctypes.c_void_p(rp), rs,
                                       ctypes.byref(n), ctypes.c_void_p(st)))
        return res, n.value

    def _count(self, fn, geometry, n: int, max_depth, rows, pixels, out_rows, out_pixels, stream, totals) -> dict:
        """The shared half of count_rays / count_rays_row_bands: ``n`` packed rows, ``geometry`` the call's
        leading arguments."""
        on_device = any(a is not None and not isinstance(a, np.ndarray) for a in (out_rows, out_pixels))
        st = _stream_handle(stream, self.device if on_device else None)
        if out_rows is None and rows:
            out_rows = np.zeros((n, 4), np.uint64)
        if out_pixels is None and pixels:
            out_pixels = np.zeros((n, self.width, 4), np.uint32)
        if not totals and out_rows is None and out_pixels is None:
            raise ValueError("nothing to count into: totals, rows and pixels are all off")

        def address(a, shape, dtype, what):
            if a is None:
                return None, 0
            if a.shape[0] < n or tuple(a.shape[1:]) != shape:
                raise ValueError(f"{what} {tuple(a.shape)} holds fewer than {n} rows of {shape}")
            # (torch's signed types of the same width serve as well: the counts are far below their sign bit)
            signed = dtype[1:]                # "uint64" -> "int64"
            _check_rows(a, signed if str(a.dtype).split(".")[-1] == signed else dtype, what)
            return _address(a) if a.shape[0] else (None, 0)

        rp, rs = address(out_rows, (4,), "uint64", "row counts")
        if out_rows is not None and rs not in (0, 32):
            raise ValueError("the row counts must be contiguous")
        pp, ps = address(out_pixels, (self.width, 4), "uint32", "pixel counts")
        t = _lib.rt_ray_counts()
        res = {}
        if totals or rp or pp:                # (no row at all: nothing to pass, the counts are zero)
            check(fn(self.h, *geometry, int(max_depth), ctypes.byref(t) if totals else None, ctypes.c_void_p(rp),
                     ctypes.c_void_p(pp), ps, ctypes.c_void_p(st)))
        if totals:
            res = {"primary": t.primary, "shadow": t.shadow, "reflect": t.reflect, "refract": t.refract,
                   "total": t.primary + t.shadow + t.reflect + t.refract}
        if out_rows is not None:
            res["rows"] = out_rows
        if out_pixels is not None:
            res["pixels"] = out_pixels
        return res

    def count_rays(self, y0: int = 0, y1: Optional[int] = None, max_depth: int = -1, rows: bool = False,
                   pixels: bool = False, out_rows=None, out_pixels=None, stream=None, totals: bool = True) -> dict:
        """rt_count_rays: the ray counts of rows [y0, y1) (default: the whole frame) of the uploaded scene, by
        the reference's definitions -- its ALGORITHMIC counts, not what the culling render kernels execute:
        ``primary`` camera rays (one per pixel; two on an anaglyph scene), ``reflect`` / ``refract``
        get_ray_color calls of those ray types, ``shadow`` = lights x rays that hit an object -- and their sum
        ``total``.  With ``rows`` also ``"rows"``: (n, 4) uint64 per-row sums in that order; with ``pixels``
        ``"pixels"``: (n, W, 4) uint32.  Both are numpy arrays, or the torch device tensors (or numpy arrays)
        passed as ``out_rows`` / ``out_pixels``; with device tensors and ``totals=False`` the call is
        asynchronous on ``stream`` (torch's current stream) and the dict holds no sums."""
        y1 = self.height if y1 is None else y1
        return self._count(lib().rt_count_rays, (int(y0), int(y1)), max(int(y1) - int(y0), 0), max_depth, rows, pixels,
                           out_rows, out_pixels, stream, totals)

    def count_rays_row_bands(self, y_first: int, band_rows: int, band_pitch: int, n_bands: int, max_depth: int = -1,
                             rows: bool = False, pixels: bool = False, out_rows=None, out_pixels=None, stream=None,
                             totals: bool = True) -> dict:
        """rt_count_rays_row_bands: count_rays for the rows of a band layout (the geometry of render_row_bands).
        The arrays hold the rows PACKED, band b row j at row b*band_rows + j of n_bands*band_rows rows; rows
        past the frame's height are not written (arrays made here hold zeros there)."""
        return self._count(lib().rt_count_rays_row_bands, (int(y_first), int(band_rows), int(band_pitch), int(n_bands)),
                           int(band_rows) * int(n_bands), max_depth, rows, pixels, out_rows, out_pixels, stream, totals)

    # rt_hit_planes in field order: (name, dtype, trailing shape after (rows, W))
    _HIT_PLANES = (("object", "int32", ()), ("distance", "float64", ()), ("shadow", "uint32", ()),
                   ("normal", "float64", (3,)))

    def _first_hits(self, fn, geometry, n: int, shadow, normal, out, stream) -> dict:
        """The shared half of first_hits / first_hits_row_bands: ``n`` packed rows, ``geometry`` the call's
        leading arguments."""
        out = dict(out or {})
        unknown = set(out) - {name for name, _, _ in self._HIT_PLANES}
        if unknown:
            raise ValueError(f"unknown first-hit planes {sorted(unknown)}")
        want = {"object": True, "distance": True, "shadow": bool(shadow) or "shadow" in out,
                "normal": bool(normal) or "normal" in out}
        made = [name for name, _, _ in self._HIT_PLANES if want[name] and out.get(name) is None]
        on_device = bool(made) or any(a is not None and not isinstance(a, np.ndarray) for a in out.values())
        st = _stream_handle(stream, self.device if on_device else None)
        if made:
            import torch
            dev = torch.device("cuda", self.device)
        planes = _lib.rt_hit_planes()
        res = {}
        for name, dtype, tail in self._HIT_PLANES:
            if not want[name]:
                continue
            a = out.get(name)
            shape = (self.width,) + tail
            if a is None:
                a = torch.empty((n,) + shape, dtype=getattr(torch, dtype), device=dev)
            elif a.shape[0] < n or tuple(a.shape[1:]) != shape:
                raise ValueError(f"{name} plane {tuple(a.shape)} holds fewer than {n} rows of {shape}")
            _check_rows(a, dtype, f"{name} plane")
            res[name] = a
            if a.shape[0] == 0:
                continue
            ptr, stride = _address(a)
            setattr(planes, name, ptr)
            setattr(planes, name + "_stride", stride)
        if n > 0:
            check(fn(self.h, *geometry, ctypes.byref(planes), ctypes.c_void_p(st)))
        return res

    def first_hits(self, y0: int = 0, y1: Optional[int] = None, shadow: bool = False, normal: bool = False, out=None,
                   stream=None) -> dict:
        """rt_first_hits: what is under every pixel of rows [y0, y1) (default: the whole frame) before any
        shading.  A dict of ``"object"`` (rows, W) int32 -- the draw index of the camera ray's nearest hit, -1 on a
        miss -- and ``"distance"`` (rows, W) float64 (inf on a miss); with ``shadow`` also ``"shadow"`` (rows, W)
        uint32, bit k set when light k's shadow ray from the hit point is occluded; with ``normal`` ``"normal"``
        (rows, W, 3) float64, the shape's raw get_normal (not normalised; zeros on a miss).  The arrays are torch
        tensors on this device, written asynchronously on ``stream`` (torch's current stream), or the arrays of
        ``out``: a dict by those names of numpy arrays or torch device tensors (a numpy array makes the call
        synchronous; naming a plane in ``out`` asks for it)."""
        y1 = self.height if y1 is None else y1
        return self._first_hits(lib().rt_first_hits, (int(y0), int(y1)), max(int(y1) - int(y0), 0), shadow, normal,
                                out, stream)

    def first_hits_row_bands(self, y_first: int, band_rows: int, band_pitch: int, n_bands: int, shadow: bool = False,
                             normal: bool = False, out=None, stream=None) -> dict:
        """rt_first_hits_row_bands: first_hits for the rows of a band layout (the geometry of render_row_bands).
        The arrays hold the rows PACKED, band b row j at row b*band_rows + j of n_bands*band_rows rows; rows past
        the frame's height are not written."""
        return self._first_hits(lib().rt_first_hits_row_bands,
                                (int(y_first), int(band_rows), int(band_pitch), int(n_bands)),
                                int(band_rows) * int(n_bands), shadow, normal, out, stream)

    def first_hits_points(self, xy, shadow: bool = False, normal: bool = False) -> dict:
        """rt_first_hits_points: the same at sample positions ``xy`` (n, 2), fractional allowed, as numpy arrays:
        ``"object"`` (n,) int32, ``"distance"`` (n,) float64, with ``shadow`` ``"shadow"`` (n,) uint32, with
        ``normal`` ``"normal"`` (n, 3) float64.  Synchronous."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        res = {"object": np.full(n, -1, np.int32), "distance": np.full(n, np.inf, np.float64)}
        if shadow:
            res["shadow"] = np.zeros(n, np.uint32)
        if normal:
            res["normal"] = np.zeros((n, 3), np.float64)
        ptr = [ctypes.c_void_p(res[k].ctypes.data) if k in res else None for k, _, _ in self._HIT_PLANES]
        check(lib().rt_first_hits_points(self.h, ctypes.c_void_p(xy.ctypes.data), n, *ptr, None))
        return res

    def record_rays(self, x: float, y: float, max_depth: int = -1, cap: int = 1 << 17):
        """rt_record_rays: (records as a RAY_RECORD_DTYPE array in callback order, pixel colour)."""
        buf = np.zeros(cap, RAY_RECORD_DTYPE)
        n = ctypes.c_int32(0)
        rgba = (ctypes.c_double * 4)()
        check(lib().rt_record_rays(self.h, float(x), float(y), int(max_depth), ctypes.c_void_p(buf.ctypes.data),
                                   cap, ctypes.byref(n), rgba))
        return buf[:min(n.value, cap)].copy(), np.array(rgba[:])

    def ray_paths_offsets(self, xy, max_depth: int = -1) -> np.ndarray:
        """rt_ray_paths_offsets: how many rays each sample position of ``xy`` (n, 2) traces (primary + reflect +
        refract), as an exclusive prefix sum: a uint64 array of n + 1, the last entry the total.  Synchronous."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        offsets = np.zeros(n + 1, np.uint64)
        total = ctypes.c_uint64(0)
        check(lib().rt_ray_paths_offsets(self.h, ctypes.c_void_p(xy.ctypes.data), n, int(max_depth),
                                         ctypes.c_void_p(offsets.ctypes.data), ctypes.byref(total), None))
        return offsets

    def ray_paths(self, xy, max_depth: int = -1) -> dict:
        """The ray debugger's records of every sample position of ``xy`` (n, 2) in one launch (rt_ray_paths_offsets,
        then rt_ray_paths into buffers of exactly the total): ``"offsets"`` uint64 (n + 1), ``"records"`` a
        RAY_RECORD_DTYPE array of offsets[n] records -- sample i's are records[offsets[i]:offsets[i + 1]] in the
        reference's callback order, the primary ray last -- and ``"rgba"`` (n, 4) float64, get_pixel's colours.
        Perspective scenes; synchronous."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        offsets = self.ray_paths_offsets(xy, max_depth)
        total = int(offsets[n])
        records = np.zeros(total, RAY_RECORD_DTYPE)
        rgba = np.zeros((n, 4), np.float64)
        check(lib().rt_ray_paths(self.h, ctypes.c_void_p(xy.ctypes.data), n, int(max_depth),
                                 ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(records.ctypes.data), total,
                                 ctypes.c_void_p(rgba.ctypes.data), None))
        return {"offsets": offsets, "records": records, "rgba": rgba}

    def render_ortho(self, axes: "OrthoAxes", y0: int = 0, y1: Optional[int] = None, f64: bool = False) -> np.ndarray:
        """rt_render_ortho rows [y0, y1) into a host array (uint8 RGBA, or float64 with ``f64``)."""
        y1 = self.height if y1 is None else y1
        out = np.empty((y1 - y0, self.width, 4), np.float64 if f64 else np.uint8)
        p8, s8, pf, sf = (None, 0, out.ctypes.data, out.strides[0]) if f64 else (out.ctypes.data, out.strides[0], None, 0)
        check(lib().rt_render_ortho(self.h, axes.axis1, axes.axis2, float(axes.dir1), float(axes.dir2),
                                    float(axes.scale), y0, y1, ctypes.c_void_p(p8), s8, ctypes.c_void_p(pf), sf,
                                    None))
        return out

    def set_kernel(self, kernel: str = "auto") -> None:
        """rt_ctx_set_option(RT_OPT_KERNEL): "auto", "mega", "deferred" or "wavefront" (same pixels;
        see rt_abi.h)."""
        v = {"auto": _lib.RT_KERNEL_AUTO, "mega": _lib.RT_KERNEL_MEGA, "deferred": _lib.RT_KERNEL_DEFERRED,
             "wavefront": _lib.RT_KERNEL_WAVEFRONT}[kernel]
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_KERNEL, v))

    def set_timing(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_TIMING): record (default) or skip the HIP event pair around every
        render launch that last_kernel_ms() reads (each timed event costs the stream ~5 us)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_TIMING, 1 if on else 0))

    def set_tile_order(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_TILE_ORDER): longest-first tile dispatch after a calibration launch
        (default) or row-major tiles (same pixels)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_TILE_ORDER, 1 if on else 0))

    def set_fast_clamp(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_FAST_CLAMP): min/max colour clamps where the host proved them exact
        (default) or the reference's compare/select clamps everywhere (same pixels)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_FAST_CLAMP, 1 if on else 0))

    def set_wavefront_cap(self, percent: int) -> None:
        """rt_ctx_set_option(RT_OPT_WAVEFRONT_CAP): rays per recursion level of the wavefront path, in
        percent of the launch's pixel slots (pixels whose tree overflows are re-rendered, same bits)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_WAVEFRONT_CAP, int(percent)))

    def set_wavefront_pairs(self, mode: int) -> None:
        """rt_ctx_set_option(RT_OPT_WAVEFRONT_PAIRS): the wavefront path's per-level tracing: 0 one wave
        walks the hierarchy for 64 rays, 1 (default) levels >= 1 as (ray, object) pairs sorted by
        object, 2 every level (same pixels)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_WAVEFRONT_PAIRS, int(mode)))

    def set_specialize(self, level: int = 1, wait: bool = True) -> None:
        """rt_ctx_set_option(RT_OPT_SPECIALIZE): 0 the precompiled kernels; 1 (the library default) the
        uploaded scene's RGBA8 / RGB8 row kernels compiled with the scene as constants (hipRTC in the
        library's background pool; same pixels); 2 its f64 and calibration kernels too.  ``wait``: block
        until the program is loaded (spec_wait), raising if it failed."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_SPECIALIZE, int(level)))
        if wait and level:
            self.spec_wait()

    def set_tile_masks(self, mode) -> None:
        """rt_ctx_set_option(RT_OPT_TILE_MASKS): per-tile object masks for the specialised reflection-only
        kernels (same pixels): 0 / False never, 1 (the default) where the geometry's calibration found them
        to pay, 2 / True for every launch that can take them."""
        v = (2 if mode else 0) if isinstance(mode, bool) else int(mode)
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_TILE_MASKS, v))

    def set_tile_records(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_TILE_RECORDS): masked launches read one dispatch record per order entry
        (the default), or the tile order and the tile-indexed mask table themselves (same pixels)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_TILE_RECORDS, 1 if on else 0))

    def set_sky_fill(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_SKY_FILL): waves of sky tiles (an empty ``prim`` word in the dispatch record)
        store BLACK and return (default on); off, the records mark no tile as sky.  Same pixels."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_SKY_FILL, 1 if on else 0))

    def set_lean_tiles(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_LEAN_TILES): the entries of a megakernel launch whose rays can meet the floor
        alone are rendered by the program's lean kernel ahead of the megakernel (default on).  Same pixels."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_LEAN_TILES, 1 if on else 0))

    def set_traced_masks(self, mode: int) -> None:
        """rt_ctx_set_option(RT_OPT_TRACED_MASKS): a record table's words narrowed once to what its entries' own
        pixels hit, by a trace pass behind the gather (same pixels): 0 never, 1 (the default) where the library
        itself picks the masked megakernel and the upload has had eight row launches, 2 and 3 for every megakernel
        launch that reads records.  The table of 1 and 3 also traces the entries with a pixel on a boxed object
        (r0's sign bit in ``tile_records``); 2 keeps those entries' predicate words."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_TRACED_MASKS, int(mode)))

    def tile_records(self) -> np.ndarray:
        """rt_ctx_tile_records: the dispatch records of the last row launch as its kernels read them, uint32
        [entries, 8]: x0 (sign bit: the entry says lean), r0 (sign bit: words 1..5 traced for every hit), prim,
        shadow[0..3], refl."""
        n = ctypes.c_uint32()
        check(lib().rt_ctx_tile_records(self.h, None, 0, ctypes.byref(n)))
        recs = np.zeros((n.value, 8), dtype=np.uint32)
        check(lib().rt_ctx_tile_records(self.h, ctypes.c_void_p(recs.ctypes.data), n.value, ctypes.byref(n)))
        return recs

    def tile_masks(self, y_first: int = 0, band_rows: Optional[int] = None, band_pitch: Optional[int] = None,
                   n_bands: int = 1) -> np.ndarray:
        """rt_ctx_tile_masks: the uploaded scene's mask table of a band launch (default: the whole frame)
        as the device computed it, uint32 [tiles, 6]."""
        band_rows = self.height - y_first if band_rows is None else band_rows
        band_pitch = band_rows if band_pitch is None else band_pitch
        tiles = ((self.width + 7) // 8) * ((band_rows * n_bands + 7) // 8)
        words = np.zeros((tiles, _lib.RT_TILEMASK_WORDS), dtype=np.uint32)
        n = ctypes.c_uint32()
        check(lib().rt_ctx_tile_masks(self.h, y_first, band_rows, band_pitch, n_bands,
                                      ctypes.c_void_p(words.ctypes.data), words.size, ctypes.byref(n)))
        assert n.value == tiles, (n.value, tiles)
        return words

    def spec_wait(self, timeout_ms: int = -1) -> bool:
        """rt_ctx_spec_wait: block until the scene-specialised program is loaded (True), or until
        ``timeout_ms`` passed (False); raises RtError when the compile failed or the guard refused it."""
        rc = check(lib().rt_ctx_spec_wait(self.h, int(timeout_ms)))
        return rc != _lib.RT_PENDING

    def set_spec_samples(self, on: bool) -> None:
        """rt_ctx_set_option(RT_OPT_SPEC_SAMPLES): let render_points and the anti-aliasing trace take the
        scene's specialised sample kernels once they are loaded (default), or always the generic ones
        (same samples)."""
        check(lib().rt_ctx_set_option(self.h, _lib.RT_OPT_SPEC_SAMPLES, 1 if on else 0))

    def spec_wait_samples(self, timeout_ms: int = -1) -> bool:
        """rt_ctx_spec_wait_samples: request the sample programs if this renderer has not yet, and block
        until they are loaded (True) or ``timeout_ms`` passed (False); raises RtError when one failed."""
        rc = check(lib().rt_ctx_spec_wait_samples(self.h, int(timeout_ms)))
        return rc != _lib.RT_PENDING

    def sample_kernel_info(self) -> str:
        """rt_ctx_sample_kernel_info: per sample path (points, aa trace) generic (and why) or specialised
        (and its resources), and what the last points / anti-aliasing trace launch ran."""
        buf = ctypes.create_string_buffer(4096)
        check(lib().rt_ctx_sample_kernel_info(self.h, buf, 4096))
        return buf.value.decode()

    def kernel_info(self) -> str:
        """rt_ctx_kernel_info: generic or scene-specialised kernels, and what the last row launch ran."""
        buf = ctypes.create_string_buffer(4096)
        check(lib().rt_ctx_kernel_info(self.h, buf, 4096))
        return buf.value.decode()

    def kernel_variant(self) -> str:
        """"spec" when the context holds scene-specialised kernels, else "generic"."""
        return "spec" if self.kernel_info().startswith("scene-specialised") else "generic"

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float()
        check(lib().rt_ctx_last_kernel_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def synchronize(self) -> None:
        check(lib().rt_ctx_synchronize(self.h))

    def free(self) -> None:
        if self.h and self.h.value:
            lib().rt_ctx_free(self.h)
            self.h = ctypes.c_void_p()

    # Contexts still alive at interpreter exit are freed by an atexit hook, registered after torch's
    # (atexit runs last-registered first) and so while the HIP runtime is still up: a context freed
    # during module teardown unloaded its specialised modules / freed its buffers after torch had
    # shut its side of the runtime down (round 4: SIGSEGV / std::bad_variant_access at exit).
    # The hook is moved to the END of the atexit list whenever a renderer is made (atexit runs the
    # last-registered first), so it still runs before hooks that torch registers once its CUDA side
    # starts; it also stops the library's compile pool (rt_spec_shutdown) so that no hipRTC compile
    # runs while the process tears the runtime down.
    @classmethod
    def _register(cls, r: "Renderer") -> None:
        import atexit
        if "_live" not in cls.__dict__:
            import weakref
            cls._live = weakref.WeakSet()
        atexit.unregister(cls.free_all)
        atexit.register(cls.free_all)
        cls._live.add(r)

    @classmethod
    def free_all(cls) -> None:
        for r in list(cls.__dict__.get("_live", ())):
            r.free()
        lib().rt_spec_shutdown()

    def __del__(self):
        if _sys.is_finalizing():
            return
        try:
            self.free()
        except Exception:
            pass


class RayTracer:
    """raytracer.rs:21-364 over the GPU path.

    Build the scene with the same calls the reference's scene parser makes, or ``load_scene``
    a DSL text; then ``get_pixel`` / ``render_lines`` as the GUI worker does."""

    def __init__(self, width: int, height: int, device: int = 0):
        self.width, self.height = width, height
        self.scene = Scene.new_default(width, height)       # RayTracer::new_default (:38-44)
        self.transformation_stack = TransformationStack()
        self.device = device
        self._renderer: Optional[Renderer] = None
        self._dirty = True
        self._max_depth = 10
        self._camera_kind = ("perspective", 0.0)

    new_default = classmethod(lambda cls, width, height, device=0: cls(width, height, device))

    # -- scene construction (raytracer.rs:72-130, 289-330) --------------------------------
    def add_test_objects(self) -> None:
        check(lib().rt_scene_add_test_objects(self.scene.h))
        self._dirty = True

    def add_texture(self, rgba8: np.ndarray) -> int:
        rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
        h, w = rgba8.shape[:2]
        self._dirty = True
        return check(lib().rt_scene_add_texture(self.scene.h, w, h, ctypes.c_void_p(rgba8.ctypes.data)))

    def _xf(self, t: Optional[MatrixTransformation]) -> _lib.rt_transformation:
        return (t or self.transformation_stack.get_transformation()).xf

    def sphere(self, center=(0, 0, 0), radius=1.0, t: Optional[MatrixTransformation] = None) -> int:
        return check(lib().rt_shape_sphere(self.scene.h, ctypes.byref(self._xf(t)), d3(center), float(radius)))

    def cube(self, center=(0, 0, 0), length=1.0, t: Optional[MatrixTransformation] = None) -> int:
        return check(lib().rt_shape_cube(self.scene.h, ctypes.byref(self._xf(t)), d3(center), float(length)))

    def plane(self, normal=(0, 1, 0), distance=1.0, t: Optional[MatrixTransformation] = None) -> int:
        return check(lib().rt_shape_plane(self.scene.h, ctypes.byref(self._xf(t)), d3(normal), float(distance)))

    def csg(self, a: int, b: int, operator: str = "union") -> int:
        op = {"union": 0, "intersection": 1, "difference": 2}[operator]
        return check(lib().rt_shape_csg(self.scene.h, op, a, b))

    def add_object(self, shape: int, material: Optional[_lib.rt_material] = None) -> None:
        check(lib().rt_scene_add_object(self.scene.h, shape, ctypes.byref(material or solid_material())))
        self._dirty = True

    def add_light(self, point, color=(0.5, 0.5, 0.5, 1.0), fade_distance=100.0) -> None:
        check(lib().rt_scene_add_light(self.scene.h, d3(point), d4(list(color) + [1.0] * (4 - len(color))),
                                       float(fade_distance)))
        self._dirty = True

    def set_camera_from_vector(self, center) -> None:
        """raytracer.rs:289-299: the centre is transformed by the stack top first."""
        c = self.transformation_stack.get_transformation().transform_vector(center)
        check(lib().rt_scene_set_camera(self.scene.h, d3(c)))
        self._dirty = True

    @property
    def max_depth(self) -> int:
        return self._max_depth

    @max_depth.setter
    def max_depth(self, d: int) -> None:
        check(lib().rt_scene_set_max_depth(self.scene.h, int(d)))
        self._max_depth = int(d)
        self._dirty = True

    def set_camera_kind(self, kind: str, eye_distance: float = 0.0) -> None:
        """The scene's Camera: "perspective" (the default), "stereoscopic" (camera.rs:82-141, two eyes side
        by side) or "anaglyph" (:143-205, red from the left eye, green and blue from the right).  Kept, like
        max_depth, across load_scene."""
        self.scene.set_camera_kind(kind, eye_distance)
        self._camera_kind = (kind, float(eye_distance))
        self._dirty = True

    def load_scene(self, text: str, time: float = 0.0, asset_dir: Optional[str] = None,
                   strict: bool = True, camera_kind: Optional[str] = None,
                   eye_distance: Optional[float] = None) -> None:
        """DebugWindow::load_ray_tracer (debug_window.rs:53-62): a fresh new_default RayTracer
        with the test light, then load_scene(text, time).  Replaces this tracer's scene.
        camera_kind / eye_distance: set_camera_kind on the new scene (the DSL has no syntax for it)."""
        if camera_kind is not None:
            if camera_kind != "perspective" and eye_distance is None:
                raise ValueError(f"camera kind {camera_kind!r} needs an eye_distance")
            self._camera_kind = (camera_kind, float(eye_distance or 0.0))
        self.scene = Scene.compile(text, time, self.width, self.height, asset_dir, strict)
        self.transformation_stack = TransformationStack()
        if self._max_depth != 10:
            check(lib().rt_scene_set_max_depth(self.scene.h, self._max_depth))
        if self._camera_kind[0] != "perspective":
            self.scene.set_camera_kind(*self._camera_kind)
        self._dirty = True

    # -- rendering ------------------------------------------------------------------------
    @property
    def renderer(self) -> Renderer:
        if self._renderer is None:
            self._renderer = Renderer(self.device)
        if self._dirty:
            self._renderer.upload(self.scene)
            self._dirty = False
        return self._renderer

    def get_pixel(self, x: float, y: float) -> np.ndarray:
        """raytracer.rs:359-363: colour (r, g, b, a) of the camera ray through (x, y)."""
        return self.renderer.render_points(np.array([[x, y]], np.float64))[0]

    def render_lines(self, line_range: Iterable[int]) -> Iterator[Tuple[int, np.ndarray]]:
        """debug_window.rs:74-87: yields (y, row of W colours as (W, 4) f64)."""
        r = self.renderer
        for y in line_range:
            yield y, r.render_rows_host(y, y + 1, f64=True)[0]

    def render_frame(self) -> np.ndarray:
        """The whole frame as RGBA8 (H, W, 4), quantised as easy_pixbuf.rs:46-53."""
        return self.renderer.render_rows_host(0, self.height)

    def count_rays(self, rows: bool = False, pixels: bool = False) -> dict:
        """The whole frame's ray counts at this tracer's max_depth (Renderer.count_rays): the reference's
        algorithmic counts -- primary, shadow, reflect, refract and their total."""
        return self.renderer.count_rays(0, self.height, self.max_depth, rows=rows, pixels=pixels)

    def first_hits(self, shadow: bool = False, normal: bool = False) -> dict:
        """The whole frame's first-hit maps (Renderer.first_hits): per pixel the object under it, its distance
        and, on request, the occluded-light bits and the shape's raw normal."""
        return self.renderer.first_hits(0, self.height, shadow=shadow, normal=normal)

    def pick(self, x: float, y: float) -> Tuple[int, float]:
        """(object, distance) under the sample position (x, y): the draw index of the camera ray's nearest hit
        and its distance, (-1, inf) on a miss (Renderer.first_hits_points)."""
        res = self.renderer.first_hits_points(np.array([[x, y]], np.float64))
        return int(res["object"][0]), float(res["distance"][0])

    def ray_paths(self, xy) -> dict:
        """The ray debugger's records of every sample position of ``xy`` (n, 2) at this tracer's max_depth
        (Renderer.ray_paths): offsets, records in callback order per sample, colours."""
        return self.renderer.ray_paths(xy, self.max_depth)

    def render_orthogonal_view_line(self, y: int, ortho_axes: "OrthoAxes") -> np.ndarray:
        """DebugWindow::render_orthogonal_view_line (debug_window.rs:166-227): (W, 4) f64 colours."""
        return _ortho_line(self, y, ortho_axes)

    def render_orthogonal_view(self, area: str = "top") -> np.ndarray:
        """A whole orthogonal preview ("top", "front", "side") as RGBA8 (H, W, 4)."""
        return self.renderer.render_ortho(OrthoAxes.from_area(area))


ORTHO_SCALE = 2.0   # ray_debugger.rs:11

# rt_ray_record (include/rt_abi.h) as a numpy dtype
RAY_RECORD_DTYPE = np.dtype([
    ("depth", "<i4"), ("ray_type", "<i4"), ("object", "<i4"), ("intersected", "<i4"), ("has_normal", "<i4"),
    ("pad", "<i4"), ("point", "<f8", 3), ("direction", "<f8", 3), ("distance", "<f8"),
    ("intersection", "<f8", 3), ("normal", "<f8", 3), ("color", "<f8", 4)])
RAY_TYPES = ("NormalRay", "ReflectionRay", "TransmissionRay")


class RayDebugger:
    """ray_debugger.rs:71-137: records every ray of one pixel (RayInfo list in callback order)."""

    def __init__(self, width: int, height: int):
        self.rays = np.zeros(0, RAY_RECORD_DTYPE)
        self.debugged_position = None
        self.width, self.height = width, height
        self.show_normals = True

    def record_rays(self, ray_tracer: "RayTracer", x: float, y: float) -> None:
        if self.debugged_position == (x, y):          # already showing these rays (:93-97)
            return
        self.debugged_position = (x, y)
        self.rays = ray_tracer.renderer.record_rays(x, y, ray_tracer.max_depth)[0]

    def record_rays_many(self, ray_tracer: "RayTracer", xy) -> np.ndarray:
        """record_rays for every sample position of ``xy`` (n, 2) in one launch (RayTracer.ray_paths): ``rays`` then
        holds every sample's records in sample order, each sample's in callback order -- what the ortho views draw
        for a scanline or a dragged region.  Returns the offsets (n + 1) of the samples' records in ``rays``."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        res = ray_tracer.ray_paths(xy)
        self.debugged_position = None if xy.shape[0] != 1 else (float(xy[0, 0]), float(xy[0, 1]))
        self.rays = res["records"]
        return res["offsets"]

    def reset_debugger(self) -> None:
        self.debugged_position = None


class OrthoAxes:
    """ray_debugger.rs:24-68: the axes of an orthogonal preview view."""

    def __init__(self, axis1: int, axis2: int, dir1: float, dir2: float, scale: float = ORTHO_SCALE):
        self.axis1, self.axis2, self.dir1, self.dir2, self.scale = int(axis1), int(axis2), dir1, dir2, scale

    @staticmethod
    def from_area(area: str) -> "OrthoAxes":
        """impl From<DrawingArea> for OrthoAxes: "top", "front" or "side"."""
        if area == "top":
            return OrthoAxes(0, 2, 1.0, -1.0)
        if area == "front":
            return OrthoAxes(0, 1, 1.0, -1.0)
        if area == "side":
            return OrthoAxes(2, 1, -1.0, -1.0)
        raise ValueError("Main view is not an orthogonal view!" if area == "main" else f"unknown area {area!r}")


class AntiAliaser:
    """antialiaser.rs:7-192: adaptive anti-aliasing of a rendered (quantised) frame.

    ``AntiAliaser(ray_tracer, threshold=None, level=None)`` takes the reference's defaults
    (0.1 and 3, antialiaser.rs:18-19); the GUI passes ANTIALIAS_THRESHOLD = 0.01 and
    ANTIALIAS_LEVEL = 3 (debug_window.rs:26-27).  The whole frame is one GPU pass (rt_antialias), a
    line one band of one row (rt_antialias_row_bands); ``ray_counter`` accumulates the sub-pixel rays traced like the reference's counter."""

    def __init__(self, ray_tracer: "RayTracer", threshold: Optional[float] = None, level: Optional[int] = None):
        self.ray_tracer = ray_tracer
        self.threshold = 0.1 if threshold is None else float(threshold)
        self.level = 3 if level is None else int(level)
        self.size = (1 << self.level) + 1
        self.ray_counter = 0

    def set_threshold(self, threshold: float) -> None:
        self.threshold = float(threshold)

    def anti_alias_frame(self, frame, f64: bool = False):
        """Every line of ``anti_alias_line_vec`` (antialiaser.rs:53-71) for y in 0..H-1, as the
        AA worker does (debug_window.rs:298-318); the last row is passed through."""
        out, rays = self.ray_tracer.renderer.antialias(frame, self.threshold, self.level, self.ray_tracer.max_depth,
                                                       f64=f64)
        self.ray_counter += rays
        return out

    def anti_alias_line_vec(self, y: int, source) -> np.ndarray:
        """``anti_alias_line_vec(y, ..)`` (antialiaser.rs:53-71): line y of the whole quantised frame
        ``source`` as its W colours, (W, 4) float64 -- one band of one row (rt_antialias_row_bands).
        Adds the line's sub-pixel rays to ``ray_counter``.  The line reads row y + 1, so y must be below
        H - 1, as the reference's worker keeps it (debug_window.rs:298)."""
        h = source.shape[0]
        if not 0 <= y < h - 1:
            raise IndexError(f"line {y} outside 0..{h - 2}: the last row has no row below it and is never anti-aliased")
        out, rays = self.ray_tracer.renderer.antialias_row_bands(source, y, 1, 1, 1, self.threshold, self.level,
                                                                 self.ray_tracer.max_depth, f64=True)
        self.ray_counter += rays
        line = out[0]
        return line if isinstance(line, np.ndarray) else line.cpu().numpy()


def _ortho_line(rt: "RayTracer", y: int, ortho_axes: OrthoAxes) -> np.ndarray:
    return rt.renderer.render_ortho(ortho_axes, y, y + 1, f64=True)[0]


def write_png(path: str, rgba8: np.ndarray, channels: int = 3) -> None:
    rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
    h, w = rgba8.shape[:2]
    check(lib().rt_write_png(path.encode(), ctypes.c_void_p(rgba8.ctypes.data), w, h, rgba8.strides[0], channels))


def read_png_rgba8(path: str) -> np.ndarray:
    p = ctypes.c_void_p()
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().rt_read_png_rgba8(path.encode(), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)))
    try:
        buf = (ctypes.c_uint8 * (w.value * h.value * 4)).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(h.value, w.value, 4).copy()
    finally:
        lib().rt_free_buffer(p)


def device_count() -> int:
    n = ctypes.c_int()
    check(lib().rt_device_count(ctypes.byref(n)))
    return n.value


def spec_compiler_info() -> Tuple[str, bool]:
    """rt_spec_compiler_info: (identity of the hipRTC the specialised programs compile with, True when
    it is the ROCm installation's own -- the only one the library lets compile them)."""
    buf = ctypes.create_string_buffer(1024)
    rocm = ctypes.c_int32()
    check(lib().rt_spec_compiler_info(buf, 1024, ctypes.byref(rocm)))
    return buf.value.decode(), bool(rocm.value)


def spec_cache_dir(path: Optional[str]) -> None:
    """rt_spec_cache_dir: the on-disk code-object cache of the specialised programs (None: none)."""
    check(lib().rt_spec_cache_dir(path.encode() if path else None))


class HwStream:
    """A HIP stream on a hardware queue of its own (rt_stream_create), usable as a torch stream
    (``.torch``, a torch.cuda.ExternalStream).  Renders meant to overlap go on such streams: plain
    torch / HIP streams share the process's few hardware queues, and two renders on one queue run
    one after the other (include/rt_abi.h rt_stream_create).

    Lifetime: close() (or ``with HwStream() as s``) synchronises and destroys the stream.  Streams
    still open when the interpreter exits are closed by an atexit hook, while the HIP runtime is
    still up: a stream left for the runtime's own teardown (__cxa_finalize) was destroyed after a
    profiler's intercept tables were gone, and rocprofv3 runs died there with SIGSEGV
    (gpurun_out/r03j_kt.err, round-3 VERDICT).  __del__ never destroys a stream during interpreter
    finalisation."""

    _live: "weakref.WeakSet[HwStream]"

    def __init__(self, device: int = 0):
        import torch
        h = ctypes.c_void_p()
        check(lib().rt_stream_create(device, ctypes.byref(h)))
        self.handle = h.value
        self.torch = torch.cuda.ExternalStream(self.handle, device=torch.device("cuda", device))
        HwStream._register(self)

    @classmethod
    def _register(cls, s: "HwStream") -> None:
        if "_live" not in cls.__dict__:
            import atexit
            import weakref
            cls._live = weakref.WeakSet()
            atexit.register(cls.close_all)
        cls._live.add(s)

    @classmethod
    def close_all(cls) -> None:
        for s in list(getattr(cls, "_live", ())):
            s.close()

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.torch.synchronize()
            lib().rt_stream_destroy(ctypes.c_void_p(self.handle))
            self.handle = None

    def __enter__(self) -> "HwStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        if _sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass
