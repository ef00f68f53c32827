"""The batched ray paths (rt_ray_paths_offsets, rt_ray_paths) timed on the MI355X (diagnostic),
built like tools/first_hits_timing.py: one process, kernel times from rt_ctx_last_kernel_ms (HIP events around each
call's kernels), the launches alternating after a warm-up, RT_OPT_SPECIALIZE 0, every buffer on the device.

  python tools/ray_paths_timing.py                  the two workloads: per call (count + scan, fill + gather) and the
                                                    same samples through the generic rt_render_points_f64, as ratios;
                                                    then 4 096 samples batched, wall clock, both calls and the copies
  python tools/ray_paths_timing.py --loop           4 096 rt_record_rays calls, wall clock (run it with --root on the
                                                    PARENT commit's tree for the ratio the batched call is held to)
  python tools/ray_paths_timing.py --stages         the calls alone, ROUNDS times, for a kernel trace that splits the
                                                    stages (rocprofv3 --kernel-trace --stats -- python ... --stages)

Expectation, written down before the first run: the count stage near 1x the points kernel (the same trace, one
4-byte store instead of four doubles); the fill above it -- it stores 160 B per ray and evaluates the normal of every
hit for the record -- and the gather a copy of 2 x 160 B per record."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package and library to load (default: this one)")
ap.add_argument("--loop", action="store_true")
ap.add_argument("--stages", action="store_true")
ap.add_argument("--rounds", type=int, default=20)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import ctypes

import numpy as np
import torch
import tinyraytracerinrust_amd as T
from tinyraytracerinrust_amd._lib import check

S = os.path.join(ROOT, "tests", "golden", "scenes")
WORKLOADS = [("globes 3840x2160 step 8", "globes", 0.0, 3840, 2160, 8),
             ("spinning_globes t 0.5 1920x1080 step 4", "spinning_globes", 0.5, 1920, 1080, 4)]


def grid(w, h, step):
    xs, ys = np.arange(0, w, step, dtype=np.float64), np.arange(0, h, step, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2))


def spread(xy, k):
    """k of the samples, evenly spread over the whole list (sky, floor and globes alike)."""
    return np.ascontiguousarray(xy[::len(xy) // k][:k])


def tracer(name, t, w, h):
    rt = T.RayTracer(w, h)
    rt.load_scene(open(os.path.join(S, name + ".scene")).read(), t, asset_dir=S)
    rt.renderer.set_specialize(0, wait=False)           # the generic kernels on both sides of every ratio
    return rt


if args.loop:
    rt = tracer("globes", 0.0, 3840, 2160)
    r, xy = rt.renderer, spread(grid(3840, 2160, 8), 4096)
    for x, y in xy[:64]:
        r.record_rays(x, y, cap=64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for x, y in xy:
        n += len(r.record_rays(x, y, cap=64)[0])
    dt = time.perf_counter() - t0
    print(f"loop of {len(xy)} rt_record_rays calls ({ROOT}): {dt * 1e3:.2f} ms wall, {dt * 1e6 / len(xy):.1f} us per call, {n} records")
    sys.exit(0)

lib = T.lib()
dev = torch.device("cuda", 0)
ok = True
for label, name, t, w, h, step in WORKLOADS:
    rt = tracer(name, t, w, h)
    r = rt.renderer
    xy_h = grid(w, h, step)
    n = len(xy_h)
    xy = torch.from_numpy(xy_h).to(dev)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rgba = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    points = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    total = int(r.ray_paths_offsets(xy_h)[-1])
    records = torch.zeros(total * 160, dtype=torch.uint8, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())

    def call_offsets():
        check(lib.rt_ray_paths_offsets(r.h, p(xy), n, -1, p(offsets), None, None))

    def call_paths():
        check(lib.rt_ray_paths(r.h, p(xy), n, -1, p(offsets), p(records), total, p(rgba), None))

    def call_points():
        check(lib.rt_render_points_f64(r.h, p(xy), n, -1, p(points), None))

    launches = {"points (generic rt_render_points_f64)": call_points, "offsets (count + scan)": call_offsets,
                "paths (fill + gather)": call_paths}
    if args.stages:
        launches.pop("points (generic rt_render_points_f64)")
    for _ in range(3):
        for f in launches.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in launches}
    for _ in range(args.rounds):
        for k, f in launches.items():
            f()
            torch.cuda.synchronize()
            ms[k].append(r.last_kernel_ms())
    print(f"{label}: {n} samples, {total} records ({total / n:.3f} per sample), {total * 160 / 1e6:.2f} MB of records")
    base = float(np.mean(ms.get("points (generic rt_render_points_f64)", [1.0])))
    for k, v in ms.items():
        print(f"  {k:40s} mean {np.mean(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({np.mean(v) / base:.3f} x points)")
    if not args.stages:
        ok = ok and torch.equal(rgba, points)              # the same colours, bit for bit
        ok = ok and int(offsets[n].item()) == total

if not args.stages:
    # 4 096 samples batched, as a host sees it: both calls, host buffers (staging and copies included), wall clock
    rt = tracer("globes", 0.0, 3840, 2160)
    r, xy_h = rt.renderer, spread(grid(3840, 2160, 8), 4096)
    for _ in range(3):
        res = r.ray_paths(xy_h)
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        res = r.ray_paths(xy_h)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"batched: {len(xy_h)} samples, {len(res['records'])} records, Renderer.ray_paths (host arrays) "
          f"mean {np.mean(wall):.3f} ms wall  min {min(wall):.3f}  max {max(wall):.3f}")
    print(f"colours equal rt_render_points_f64 bit for bit and the totals agree: {ok}")
sys.exit(0 if ok else 1)
