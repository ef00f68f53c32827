"""The two-eye cameras on the GPU: StereoscopicCamera and AnaglyphCamera (camera.rs:82-205) through every
get_pixel path of the C ABI, against frames composed from the CPU oracle's perspective renders at the two
eye positions (tests/stereo_refs.py).  RGBA8 / RGB8 frames are bit-identical; f64 colours agree to 1e-9
(device acos / sin, as tests/test_gpu_parity.py).  Every pixel of every frame is compared."""
import numpy as np
import pytest

from tests.conftest import SCENES, scene_text
from tests.stereo_refs import EYE_DISTANCE, point_reference, reference

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
KINDS = ["stereoscopic", "anaglyph"]
# (scene, time, depth): reflection-only and textured; refraction chains; ray trees
SCENE_CASES = [("globes", 0.1, 10), ("spinning_globes", 0.1, 10), ("fractal", 0.0, 4)]
SIZES = [(40, 24), (37, 19)]        # 37x19: odd width, height no multiple of 8, w = 18 inside a tile column


@pytest.fixture(scope="module")
def T():
    import torch
    import tinyraytracerinrust_amd as T
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return T


def tracer(T, name, time, W, H, depth, kind, eye_distance=EYE_DISTANCE):
    rt = T.RayTracer(W, H)
    rt.max_depth = depth
    rt.load_scene(scene_text(name), time, asset_dir=SCENES, camera_kind=kind, eye_distance=eye_distance)
    return rt


def check_frames(r, ref_f, ref_u8, label, f64=True):
    H = ref_u8.shape[0]
    gu = r.render_rows_host(0, H)
    d = np.abs(gu.astype(np.int16) - ref_u8.astype(np.int16))
    print(f"{label}: u8 max|d|={d.max()} exact={100 * float(np.mean(d == 0)):.4f}%")
    assert np.array_equal(gu, ref_u8), f"{label}: {int((d > 0).sum())} channels differ (max {d.max()} LSB)"
    if f64:
        gf = r.render_rows_host(0, H, f64=True)
        fd = np.abs(gf - ref_f)
        print(f"{label}: f64 max|d|={np.nanmax(fd):.3e}")
        assert np.array_equal(np.isnan(gf), np.isnan(ref_f))
        assert np.nanmax(fd) <= F64_TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name,time,depth", SCENE_CASES)
def test_small_frames_generic(T, worldmap, name, time, depth, W, H, kind):
    ref_f, ref_u8 = reference(name, time, W, H, depth, kind)
    r = tracer(T, name, time, W, H, depth, kind).renderer
    check_frames(r, ref_f, ref_u8, f"{name} {W}x{H} {kind}")
    assert "last launch: view megakernel" in r.kernel_info() and "specialised" not in r.kernel_info().split("last launch")[1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name,time,depth", SCENE_CASES[:2])
def test_small_frames_specialised(T, worldmap, name, time, depth, W, H, kind):
    ref_f, ref_u8 = reference(name, time, W, H, depth, kind)
    r = tracer(T, name, time, W, H, depth, kind).renderer
    r.set_specialize(2)                     # waits for the program (one per scene: the camera is an argument)
    check_frames(r, ref_f, ref_u8, f"{name} {W}x{H} {kind} specialised")
    assert "last launch: view megakernel (specialised)" in r.kernel_info(), r.kernel_info()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rgb", [False, True])
def test_bands(T, worldmap, kind, rgb):
    import torch
    W = H = 40
    _, ref_u8 = reference("globes", 0.1, W, H, 10, kind)
    r = tracer(T, "globes", 0.1, W, H, 10, kind).renderer
    world, rank, band = 2, 1, 8
    rows = [y for y in range(H) if (y // band) % world == rank]          # rank 1 of 2, 8-row cyclic bands
    n_bands = -(-len(rows) // band)
    out = torch.zeros((n_bands * band, W, 3 if rgb else 4), dtype=torch.uint8, device="cuda")
    r.render_row_bands(rank * band, band, world * band, n_bands, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:len(rows)]
    want = ref_u8[rows][..., :3] if rgb else ref_u8[rows]
    assert np.array_equal(got, want)


def test_points_stereoscopic(T, worldmap):
    W, H = 37, 19
    w = W // 2
    xy = [(x, y) for x in (w - 0.5, float(w), w + 0.25, W - 0.5, 0.0) for y in (0.0, 7.5, 18.0)]
    want = point_reference("globes", 0.1, W, H, 10, "stereoscopic", xy)
    rt = tracer(T, "globes", 0.1, W, H, 10, "stereoscopic")
    got = rt.renderer.render_points(np.array(xy))
    assert np.max(np.abs(got - want)) <= F64_TOL
    one = rt.scene.trace_pixel(w + 0.25, 7.5)
    assert np.max(np.abs(one - want[xy.index((w + 0.25, 7.5))])) <= F64_TOL


def test_points_anaglyph(T, worldmap):
    W, H = 40, 24
    xy = [(0.0, 0.0), (12.25, 9.5), (19.5, 12.0), (27.75, 15.125), (39.5, 23.5), (20.0, 20.0)]
    for name, time, depth in (("globes", 0.1, 10), ("fractal", 0.0, 4)):
        want = point_reference(name, time, W, H, depth, "anaglyph", xy)
        rt = tracer(T, name, time, W, H, depth, "anaglyph")
        got = rt.renderer.render_points(np.array(xy))
        assert np.max(np.abs(got - want)) <= F64_TOL, name
        assert (got[:, 3] == 1.0).all()
    one = rt.scene.trace_pixel(12.25, 9.5, max_depth=4)
    assert np.max(np.abs(one - want[1])) <= F64_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_ordered_path(T, worldmap, kind):
    W, H = 512, 264                          # >= 2048 entries over the two views: calibration, then ordered
    _, ref_u8 = reference("globes", 0.1, W, H, 10, kind)
    r = tracer(T, "globes", 0.1, W, H, 10, kind).renderer
    for launch in ("calibration", "ordered", "ordered again"):
        assert np.array_equal(r.render_rows_host(0, H), ref_u8), launch


def test_anaglyph_without_eye_distance_is_the_perspective_frame(T):
    W, H = 512, 264
    plain = tracer(T, "globes", 0.1, W, H, 10, None).renderer.render_rows_host(0, H)
    r = tracer(T, "globes", 0.1, W, H, 10, "anaglyph", eye_distance=0.0).renderer
    r.set_specialize(2)
    for _ in range(2):                       # the calibration launch, then an ordered one
        assert np.array_equal(r.render_rows_host(0, H), plain)
        assert "view megakernel (specialised)" in r.kernel_info()


@pytest.mark.parametrize("kind", KINDS)
def test_context_state_across_uploads(T, worldmap, kind):
    from tinyraytracerinrust_amd.raytracer import Scene
    W, H = 512, 264
    _, ref_u8 = reference("globes", 0.1, W, H, 10, kind)
    persp = Scene.compile(scene_text("globes"), 0.1, W, H, asset_dir=SCENES)
    two = Scene.compile(scene_text("globes"), 0.1, W, H, asset_dir=SCENES)
    two.set_camera_kind(kind, EYE_DISTANCE)
    fresh = T.Renderer()
    fresh.upload(persp)
    want = fresh.render_rows_host(0, H)
    r = T.Renderer()
    r.upload(two)
    for _ in range(2):
        assert np.array_equal(r.render_rows_host(0, H), ref_u8)
    r.upload(persp)                          # the same structure, another camera kind: as on a fresh context
    for _ in range(2):
        assert np.array_equal(r.render_rows_host(0, H), want)
        assert "view" not in r.kernel_info().split("last launch")[1]
    r.upload(two)                            # and the other way round
    for _ in range(2):
        assert np.array_equal(r.render_rows_host(0, H), ref_u8)


@pytest.mark.parametrize("kind", KINDS)
def test_other_calls(T, worldmap, kind):
    from tinyraytracerinrust_amd.raytracer import OrthoAxes
    W, H = 40, 24
    _, ref_u8 = reference("globes", 0.1, W, H, 10, kind)
    r = tracer(T, "globes", 0.1, W, H, 10, kind).renderer
    with pytest.raises(T.RtError) as e:
        r.antialias(np.ascontiguousarray(ref_u8))
    assert e.value.status == -6
    with pytest.raises(T.RtError) as e:
        r.record_rays(3.0, 4.0)
    assert e.value.status == -6
    with pytest.raises(T.RtError) as e:
        r.tile_masks()
    assert e.value.status == -6
    plain = tracer(T, "globes", 0.1, W, H, 10, None).renderer
    axes = OrthoAxes.from_area("top")
    assert np.array_equal(r.render_ortho(axes), plain.render_ortho(axes))
    for kernel in ("deferred", "wavefront", "auto"):
        r.set_kernel(kernel)
        assert np.array_equal(r.render_rows_host(0, H), ref_u8), kernel
    r.set_tile_masks(2)
    assert np.array_equal(r.render_rows_host(0, H), ref_u8)
    assert "tile masks: off" in r.kernel_info()
