"""Time the anti-aliasing pass and rt_render_points_f64 (diagnostic).

Without arguments: the anti-aliasing pass on the 1080p and 4K globes frames through the package.

--ab: an interleaved A/B in ONE process of RT_OPT_SPEC_SAMPLES 0 and 1 (the generic and the scene-specialised
sample kernels, spec_text.cpp rt_spec_points / rt_spec_aa) and, with --parent LIB, of another build of the library
(one without the option: the parent commit's), each variant through its own ctypes handle, context and upload
as tools/ab_libs.py does.  Per round every variant runs one anti-aliasing pass of the config's frame (wall time
with a device synchronisation, and the pass's kernel span from rt_ctx_last_kernel_ms) and --point-launches
launches of rt_render_points_f64 on --points random positions (device pointers, one event pair around them).
Prints per variant the median and every sample, and checks that all variants wrote the same bytes.
usage: python tools/aa_timing.py --ab [--parent LIB [--parent-samples 0|1]] [--reverse] [--config globes4k|globes1080|anim1080] [--threshold 0.01]
       [--level 3] [--rounds 7] [--points 1000000]
The per-pass times of the trace kernels come from a kernel trace of such a run (tools/aa_passes.py)."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = os.path.join(ROOT, "tests", "golden", "scenes")
# anim1080: the anim120 benchmark's scene (spinning_globes, refraction chains) at one of its times
CONFIGS = {"globes4k": ("globes", 0.0, 3840, 2160), "globes1080": ("globes", 0.0, 1920, 1080),
           "anim1080": ("spinning_globes", 0.5, 1920, 1080)}
RT_OPT_TIMING, RT_OPT_SPECIALIZE, RT_OPT_SPEC_SAMPLES = 1, 6, 9


def plain():
    import torch
    import tinyraytracerinrust_amd as T
    for W, H in [(1920, 1080), (3840, 2160)]:
        rt = T.RayTracer(W, H)
        rt.load_scene(open(os.path.join(S, "globes.scene")).read(), 0.0, asset_dir=S)
        r = rt.renderer
        frame = r.render_rows(0, H)
        out, rays = r.antialias(frame, 0.01, 3)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            out, rays = r.antialias(frame, 0.01, 3, out=out)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"AA globes {W}x{H}: {min(ts):.2f} ms wall (kernels {r.last_kernel_ms():.2f} ms), "
              f"{rays} sub-pixel rays = {rays / (W * H):.3f}/px, {rays / (min(ts) * 1e-3) / 1e6:.0f} Mrays/s", flush=True)


def med(v):
    w = sorted(v)
    return w[len(w) // 2]


def ab(a):
    import torch
    scene, t, W, H = CONFIGS[a.config]
    text = open(os.path.join(S, scene + ".scene")).read().encode()
    here = os.path.join(ROOT, "tinyraytracerinrust_amd", "librt_mi355x.so")
    variants = ([("parent", a.parent, a.parent_samples)] if a.parent else []) + [("samples 0", here, 0), ("samples 1", here, 1)]
    if a.reverse:
        variants.reverse()
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    g = torch.Generator().manual_seed(1)
    xy = (torch.rand((a.points, 2), generator=g, dtype=torch.float64) * torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)).cuda()
    V = []
    for label, path, samples in variants:
        L = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL)
        L.rt_ctx_spec_wait.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.rt_antialias.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.rt_render_points_f64.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render_rows.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.rt_ctx_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        sc, cx = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.rt_scene_compile(text, S.encode(), ctypes.c_double(t), W, H, ctypes.byref(sc)) == 0
        assert L.rt_ctx_create(0, ctypes.byref(cx)) == 0
        assert L.rt_ctx_set_option(cx, RT_OPT_SPECIALIZE, 1) == 0
        if samples >= 0:
            assert L.rt_ctx_set_option(cx, RT_OPT_SPEC_SAMPLES, samples) == 0
        assert L.rt_ctx_upload(cx, sc) == 0
        assert L.rt_ctx_spec_wait(cx, -1) == 0
        if samples >= 0:
            L.rt_ctx_sample_kernel_info.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
            L.rt_ctx_spec_wait_samples.argtypes = [ctypes.c_void_p, ctypes.c_int32]
            assert L.rt_ctx_spec_wait_samples(cx, -1) == 0
        frame = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        for _ in range(2):                                   # calibration, then the ordered launch
            assert L.rt_render_rows(cx, 0, H, -1, frame.data_ptr(), W * 4, sp) == 0
        torch.cuda.synchronize()
        V.append(dict(label=label, L=L, cx=cx, frame=frame, out=torch.zeros_like(frame), samples=samples,
                      pts=torch.zeros((a.points, 4), dtype=torch.float64, device="cuda"), wall=[], kern=[], points=[], rays=0))

    def antialias(v):
        rays = ctypes.c_uint64(0)
        assert v["L"].rt_antialias(v["cx"], v["frame"].data_ptr(), W * 4, a.threshold, a.level, -1, v["out"].data_ptr(), W * 4,
                                   None, 0, ctypes.byref(rays), sp) == 0
        v["rays"] = rays.value

    def points(v):
        assert v["L"].rt_render_points_f64(v["cx"], xy.data_ptr(), a.points, -1, v["pts"].data_ptr(), sp) == 0
    for v in V:                                              # warm-up (the first pass allocates)
        antialias(v)
        points(v)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for v in V:
            antialias(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            antialias(v)
            torch.cuda.synchronize()
            v["wall"].append((time.perf_counter() - t0) * 1e3)
            ms = ctypes.c_float()
            assert v["L"].rt_ctx_last_kernel_ms(v["cx"], ctypes.byref(ms)) == 0
            v["kern"].append(ms.value)
        for v in V:
            assert v["L"].rt_ctx_set_option(v["cx"], RT_OPT_TIMING, 0) == 0
            points(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.point_launches):
                points(v)
            e1.record(st)
            torch.cuda.synchronize()
            v["points"].append(e0.elapsed_time(e1) / a.point_launches)
            assert v["L"].rt_ctx_set_option(v["cx"], RT_OPT_TIMING, 1) == 0
    for v in V[1:]:
        assert torch.equal(v["frame"], V[0]["frame"]) and torch.equal(v["out"], V[0]["out"]), f"{v['label']}: frames differ"
        assert torch.equal(v["pts"].view(torch.int64), V[0]["pts"].view(torch.int64)), f"{v['label']}: points differ"
    print(f"{a.config}: {scene} t={t} {W}x{H}, threshold {a.threshold}, level {a.level}: {V[0]['rays']} sub-pixel rays per pass; "
          f"{a.points} random points per launch; medians of {a.rounds} interleaved rounds (every variant wrote the same bytes)")
    for v in V:
        if v["samples"] >= 0:
            buf = ctypes.create_string_buffer(4096)
            v["L"].rt_ctx_sample_kernel_info(v["cx"], buf, 4096)
            print(f"  [{v['label']}] {buf.value.decode()}")
    for key, what in (("wall", "AA pass, ms wall"), ("kern", "AA pass, ms kernel span"), ("points", "points launch, ms")):
        for v in V:
            print(f"  {what:24s} {v['label']:10s} {med(v[key]):8.4f}  ({' '.join(f'{x:.4f}' for x in v[key])})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--parent", default="")
    ap.add_argument("--parent-samples", type=int, default=-1, choices=[-1, 0, 1],
                    help="RT_OPT_SPEC_SAMPLES for the parent build, set and waited for as for this one (-1: a build without "
                         "the option; one with it then runs the generic kernels until its own request has compiled)")
    ap.add_argument("--reverse", action="store_true", help="the variants in the opposite order, within every round")
    ap.add_argument("--config", default="globes4k", choices=sorted(CONFIGS))
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--point-launches", type=int, default=5)
    a = ap.parse_args()
    ab(a) if a.ab else plain()
