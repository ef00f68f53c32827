"""One two-eye launch against two perspective launches (interleaved, tools/ab_libs.py's arrangement): a
stereoscopic or anaglyph frame of globes.scene rendered by THIS library in one launch, against the two
perspective frames at the same eye positions (the eye scenes: `set camera(<exact decimals>)` appended)
rendered by the library given as BASE (a build of the parent commit; default: this library).  Specialised
kernels (RT_OPT_SPECIALIZE 1, waited for), RT_OPT_TIMING off, one stream; ms per frame from one event pair
around --frames launches, median over --rounds.  The two-eye frame is also checked byte for byte against
the frame composed from BASE's two.
usage: python tools/stereo_ab.py [--base LIB] [--kind anaglyph|stereoscopic] [--size WxH] [--depth D]
                                 [--eye-distance D] [--rounds N] [--base-masks 0|1|2]
       python tools/stereo_ab.py --pmc-frames N [--kind ...|perspective]   N launches of one kind only, for a
           counter pass:  rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR -o run -- python tools/stereo_ab.py ..."""
import argparse
import ctypes
import os
import sys
import time
from decimal import Decimal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = os.path.join(ROOT, "tests", "golden", "scenes")
KINDS = {"perspective": 0, "stereoscopic": 1, "anaglyph": 2}


def exact(v):
    return ("-" if v < 0 else "") + format(Decimal(abs(v)), "f")


def load(path):
    L = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL)
    L.rt_ctx_spec_wait.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    return L


def context(L, text, W, H, kind=0, eye_distance=0.0, masks=-1):
    sc, cx = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.rt_scene_compile(text.encode(), S.encode(), ctypes.c_double(0.0), W, H, ctypes.byref(sc)) == 0
    if kind:
        assert L.rt_scene_set_camera_kind(sc, kind, ctypes.c_double(eye_distance)) == 0
    assert L.rt_ctx_create(0, ctypes.byref(cx)) == 0
    assert L.rt_ctx_set_option(cx, 6, 1) == 0                      # RT_OPT_SPECIALIZE 1
    if masks >= 0:
        assert L.rt_ctx_set_option(cx, 8, masks) == 0              # RT_OPT_TILE_MASKS
    assert L.rt_ctx_upload(cx, sc) == 0
    assert L.rt_ctx_spec_wait(cx, -1) == 0
    assert L.rt_ctx_set_option(cx, 1, 0) == 0                      # RT_OPT_TIMING off, as bench.py
    return sc, cx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=os.path.join(ROOT, "tinyraytracerinrust_amd", "librt_mi355x.so"))
    ap.add_argument("--kind", default="anaglyph", choices=sorted(KINDS))
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--eye-distance", type=float, default=6.5)
    ap.add_argument("--base-masks", type=int, default=-1, help="RT_OPT_TILE_MASKS of the perspective contexts (-1: the default)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--pmc-frames", type=int, default=0)
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.size.lower().split("x"))
    text = open(os.path.join(S, "globes.scene")).read()
    new = load(os.path.join(ROOT, "tinyraytracerinrust_amd", "librt_mi355x.so"))
    kind = KINDS[a.kind]
    st = torch.cuda.current_stream()
    sc, cx = context(new, text, W, H, kind, a.eye_distance)

    def launcher(L, cx, out, h):
        args = (cx, 0, h, a.depth, ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(out.stride(0)), ctypes.c_void_p(st.cuda_stream))
        return lambda: L.rt_render_rows(*args)

    frame = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    two = launcher(new, cx, frame, H)
    if a.pmc_frames:
        for _ in range(a.pmc_frames + 1):                           # the first launch calibrates (generic kernel)
            assert two() == 0
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(4096)
        new.rt_ctx_kernel_info(cx, buf, 4096)
        print(a.kind, buf.value.decode().split("; last launch")[1])
        return
    assert kind, "--kind perspective is for --pmc-frames"
    base = load(a.base)
    w = W // 2 if a.kind == "stereoscopic" else W
    eyes, outs, runs = [], [], []
    for i in (0, 1):
        cam = (ctypes.c_double * 13)()
        assert new.rt_scene_get_camera_eye(sc, i, cam) == 0
        eye_text = text.rstrip("\n") + "\nset camera(<" + ", ".join(exact(v) for v in cam[0:3]) + ">)\n"
        _, ecx = context(base, eye_text, w, H, masks=a.base_masks)
        outs.append(torch.zeros((H, w, 4), dtype=torch.uint8, device="cuda"))
        runs.append(launcher(base, ecx, outs[i], H))
        eyes.append(list(cam[0:3]))
    runs.append(two)
    tag = "base" if a.base_masks < 0 else f"base, RT_OPT_TILE_MASKS {a.base_masks}"
    names = [f"left eye, perspective ({tag})", f"right eye, perspective ({tag})", a.kind + " (this library, one launch)"]
    for r in runs:
        assert r() == 0                                             # calibration
    torch.cuda.synchronize()
    ts = time.perf_counter()
    while time.perf_counter() - ts < 0.3:
        for r in runs:
            r()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        two()
    torch.cuda.synchronize()
    n = a.frames or max(20, int(0.08 / ((time.perf_counter() - t0) / 10)))
    res = [[] for _ in runs]
    for _ in range(a.rounds):
        for i, r in enumerate(runs):
            for _ in range(3):
                r()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(n):
                r()
            e1.record(st)
            torch.cuda.synchronize()
            res[i].append(e0.elapsed_time(e1) / n)
    L8, R8 = outs
    if a.kind == "anaglyph":
        want = R8.clone()
        want[..., 0] = L8[..., 0]
    else:
        want = torch.cat([R8, L8], dim=1)
        if W % 2:
            want = torch.cat([want, frame[:, W - 1:]], dim=1)       # the odd column has no perspective counterpart here
    if not torch.equal(frame, want):
        raise SystemExit(f"{a.kind}: the frame differs from the two perspective frames' composition")
    print(f"globes.scene {W}x{H} depth {a.depth}, {a.kind}, eye distance {a.eye_distance}, eyes {eyes}; specialised kernels, "
          f"{n} frames per measurement, ms per frame, median of {a.rounds}; frame == composition of the two: yes")
    med = []
    for name, v in zip(names, res):
        s = sorted(v)
        med.append(s[len(s) // 2])
        print(f"  {med[-1]:.4f}  (min {s[0]:.4f} max {s[-1]:.4f}: {' '.join(f'{x:.4f}' for x in v)})  {name}", flush=True)
    print(f"  t_L + t_R = {med[0] + med[1]:.4f} ms, one launch = {med[2]:.4f} ms ({100 * (med[2] / (med[0] + med[1]) - 1):+.2f} %)")
    print(f"  base = {a.base}")


if __name__ == "__main__":
    main()
