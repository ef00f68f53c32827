"""Headless driver: compile -> upload -> render -> (gather) -> PNG.

    python -m tinyraytracerinrust_amd render SCENE [--size WxH] [--time T | --frame F]
                                          [--depth D] [--gpus N] [-o out.png]
                                          [--camera {perspective,stereoscopic,anaglyph} --eye-distance D]
                                          [--antialias [--aa-threshold T] [--aa-level L]]
                                          [--count-rays] [--ray-map map.png]
                                          [--object-map o.png] [--depth-map d.png] [--normal-map n.png]
                                          [--shadow-map s.png]
                                          [--ray-paths paths.npz [--ray-paths-step N]]

Replaces the reference's entry point and its GUI load path for this purpose: ``main()`` only
starts the GTK application (src/main.rs:7-9), which builds a RayTracer per frame with
``time = frame / 300`` (src/raydebugger/debug_window.rs:53-62, gui.rs:20) and renders it row by
row into a cairo surface (debug_window.rs:74-87, 147-164).  Here the frame is rendered by the HIP
kernels and written as a PNG of exactly the bytes the GUI would show, ``(c * 255.0) as u8``
(easy_pixbuf.rs:46-53).  SCENE is a .scene path; texture names resolve against its directory
(``--assets`` overrides), like the reference's CWD-relative ``texture("worldmap.png")``.

``--gpus N`` (N > 1) renders the frame row-tiled over N GPUs, one process per GPU, assembled by one
RCCL all-gather (tinyraytracerinrust_amd/distributed.py); started without torch.distributed.run it
launches its own N ranks.  Phase times go to stderr as one JSON line.  There is no CPU path: without
a HIP device the command fails.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time


HIT_MAP_FLAGS = ("--object-map", "--depth-map", "--normal-map", "--shadow-map")


def _parse(argv):
    ap = argparse.ArgumentParser(prog="python -m tinyraytracerinrust_amd", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("render", help="render one frame of a .scene file to a PNG")
    r.add_argument("scene", help="path of a .scene file")
    r.add_argument("--size", default="480x360", help="WxH (the GUI default is 480x360, gui.rs:17-18)")
    g = r.add_mutually_exclusive_group()
    g.add_argument("--time", type=float, default=None, help="the scene's global `time` (default 0)")
    g.add_argument("--frame", type=int, default=None, help="GUI frame number: time = frame / 300")
    r.add_argument("--depth", type=int, default=-1, help="max_depth (default: the scene's, 10)")
    r.add_argument("--gpus", type=int, default=1)
    r.add_argument("--layout", default="cyclic", choices=["cyclic", "contiguous"])
    r.add_argument("--band", type=int, default=8)
    r.add_argument("--assets", default=None, help="directory textures resolve against (default: the scene's)")
    r.add_argument("--channels", type=int, default=3, choices=[3, 4], help="PNG channels (RGB or RGBA)")
    r.add_argument("--camera", default="perspective", choices=["perspective", "stereoscopic", "anaglyph"],
                   help="the scene's Camera (camera.rs): stereoscopic = two eyes side by side, anaglyph = red/cyan")
    r.add_argument("--eye-distance", type=float, default=None,
                   help="distance between the two eyes, scene units (required for stereoscopic / anaglyph)")
    r.add_argument("--antialias", action="store_true",
                   help="run the adaptive anti-aliasing pass over the rendered frame (antialiaser.rs; the GUI's "
                        "\"Anti-alias\" button); with --gpus N every rank anti-aliases the bands it rendered")
    r.add_argument("--aa-threshold", type=float, default=0.01,
                   help="mean |dRGBA| above which a cell subdivides (the GUI's ANTIALIAS_THRESHOLD, debug_window.rs:26)")
    r.add_argument("--aa-level", type=int, default=3,
                   help="subdivision levels, 0..4 (the GUI's ANTIALIAS_LEVEL, debug_window.rs:27)")
    r.add_argument("--count-rays", action="store_true",
                   help="count the frame's rays on the GPU by the reference's definitions (its algorithmic counts: "
                        "primary, shadow, reflect, refract; rt_count_rays) and report them in the JSON line; with "
                        "--gpus N every rank counts the bands it rendered")
    r.add_argument("--ray-map", default=None, metavar="PATH",
                   help="write the rays per pixel as a grey PNG, floor(255 * n / max n); implies --count-rays; "
                        "not with --gpus > 1 (no rank holds the whole map)")
    r.add_argument("--object-map", default=None, metavar="PATH",
                   help="write the object under each pixel as a grey PNG (rt_first_hits): a miss 0, object o "
                        "1 + o scaled to 1..255 over the scene's object count; one GPU, not with --camera anaglyph")
    r.add_argument("--depth-map", default=None, metavar="PATH",
                   help="write the first hit's distance as a grey PNG: the nearest white, the farthest dark grey, "
                        "misses black; one GPU, not with --camera anaglyph")
    r.add_argument("--normal-map", default=None, metavar="PATH",
                   help="write the first hit's normal as an RGB PNG, normalised * 0.5 + 0.5, misses black; one GPU, "
                        "not with --camera anaglyph")
    r.add_argument("--shadow-map", default=None, metavar="PATH",
                   help="write the share of the scene's lights each first hit can see as a grey PNG, misses black; "
                        "one GPU, not with --camera anaglyph")
    r.add_argument("--ray-paths", default=None, metavar="PATH.npz",
                   help="write the ray debugger's records of the pixel centres of every N-th column and row "
                        "(rt_ray_paths) as an .npz of xy, offsets and records; one GPU, --camera perspective")
    r.add_argument("--ray-paths-step", type=int, default=8, metavar="N",
                   help="the N of --ray-paths (default 8)")
    r.add_argument("-o", "--output", default="out.png")
    a = ap.parse_args(argv)
    for flag in HIT_MAP_FLAGS:
        if getattr(a, flag[2:].replace("-", "_")) is None:
            continue
        if a.gpus > 1:
            ap.error(f"{flag} is not built for --gpus > 1 (no rank holds the whole map)")
        if a.camera == "anaglyph":
            ap.error(f"{flag} is not built for --camera anaglyph (a pixel there has two first hits, one per eye)")
    if a.ray_paths is not None:
        if a.gpus > 1:
            ap.error("--ray-paths is not built for --gpus > 1 (the records are one rank's launch)")
        if a.camera != "perspective":
            ap.error(f"--ray-paths is not built for --camera {a.camera} (the recording traces perspective samples)")
        if a.ray_paths_step < 1:
            ap.error("--ray-paths-step must be >= 1")
    if a.ray_map is not None:
        if a.gpus > 1:
            ap.error("--ray-map is not built for --gpus > 1 (no rank holds the whole map)")
        a.count_rays = True
    if a.camera != "perspective" and a.eye_distance is None:
        ap.error(f"--camera {a.camera} needs --eye-distance (the reference constructs neither camera: no default)")
    if a.antialias and a.camera != "perspective":
        ap.error(f"--antialias is not built for --camera {a.camera} (the pass traces perspective sub-pixels)")
    if not 0 <= a.aa_level <= 4:
        ap.error("--aa-level must be in 0..4")
    if a.aa_threshold != a.aa_threshold:
        ap.error("--aa-threshold must be a number")
    try:
        w, h = a.size.lower().split("x")
        a.width, a.height = int(w), int(h)
    except ValueError:
        ap.error(f"--size must be WxH, not {a.size!r}")
    if a.width <= 0 or a.height <= 0:
        ap.error("--size must be positive")
    if a.gpus < 1:
        ap.error("--gpus must be >= 1")
    if a.band < 1:
        ap.error("--band must be >= 1")
    a.t = a.frame / 300.0 if a.frame is not None else (a.time or 0.0)
    return a


def _self_launch(argv, gpus: int) -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "tinyraytracerinrust_amd"] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def hit_maps(a, planes, n_objects: int, n_lights: int):
    """The first-hit maps the command line asked for, as (path, uint8 image) pairs from rt_first_hits' planes
    (host arrays): grey (H, W) images, the normal map RGBA (H, W, 4).  Misses are black in every map."""
    import numpy as np
    obj = planes["object"]
    hit = obj >= 0
    if a.object_map is not None:
        # object o -> (1 + o) * 255 / N, never below 1: 1..255 over the scene's N objects, a miss 0
        grey = np.maximum((obj.astype(np.int64) + 1) * 255 // max(n_objects, 1), 1)
        yield a.object_map, np.where(hit, grey, 0).astype(np.uint8)
    if a.depth_map is not None:
        # the nearest finite distance white (255), the farthest dark grey (64), linear in between
        d = planes["distance"]
        fin = hit & np.isfinite(d)
        grey = np.zeros(d.shape, np.uint8)
        if fin.any():
            lo, hi = d[fin].min(), d[fin].max()
            share = (d[fin] - lo) / (hi - lo) if hi > lo else np.zeros(int(fin.sum()))
            grey[fin] = np.floor(255.0 - share * (255.0 - 64.0)).astype(np.uint8)
        yield a.depth_map, grey
    if a.normal_map is not None:
        n = planes["normal"]
        length = np.sqrt((n * n).sum(axis=-1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            unit = np.where(np.isfinite(length) & (length > 0.0), n / length, 0.0)
        rgb = np.floor(np.clip(unit * 0.5 + 0.5, 0.0, 1.0) * 255.0).astype(np.uint8)
        img = np.zeros(obj.shape + (4,), np.uint8)
        img[..., :3] = np.where(hit[..., None], rgb, 0)
        img[..., 3] = 255
        yield a.normal_map, img
    if a.shadow_map is not None:
        # the share of the scene's lights the hit can see: lights - occluded bits, over lights
        sh = planes["shadow"].astype(np.uint64)
        occluded = np.zeros(sh.shape, np.int64)
        for k in range(min(n_lights, 32)):
            occluded += ((sh >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
        grey = (n_lights - occluded) * 255 // n_lights if n_lights > 0 else np.full(sh.shape, 255, np.int64)
        yield a.shadow_map, np.where(hit, grey, 0).astype(np.uint8)


def ray_paths_samples(width: int, height: int, step: int):
    """--ray-paths' sample positions: the pixel centres of every step-th column and row, row-major, (n, 2) f64."""
    import numpy as np
    xs, ys = np.arange(0, width, step, dtype=np.float64), np.arange(0, height, step, dtype=np.float64)
    return np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)


def render(a) -> dict:
    import numpy as np
    import torch
    import torch.distributed as dist
    from . import distributed as D
    from .raytracer import Scene, Renderer, write_png

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: the render path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    times = {}
    t0 = time.perf_counter()
    with open(a.scene) as f:
        text = f.read()
    assets = a.assets or os.path.dirname(os.path.abspath(a.scene))
    scene = Scene.compile(text, a.t, a.width, a.height, asset_dir=assets, strict=False)
    if scene.status:
        print(f"scene parse error (rendering the default scene, as the reference does): {scene.error}",
              file=sys.stderr)
    if a.camera != "perspective":
        scene.set_camera_kind(a.camera, a.eye_distance)
    times["compile_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    r = Renderer(local)
    r.upload(scene)
    torch.cuda.synchronize(dev)
    times["upload_ms"] = (time.perf_counter() - t0) * 1e3
    W, H = a.width, a.height
    t0 = time.perf_counter()
    if world == 1:
        frame = r.render_rows(0, H, max_depth=a.depth)
        torch.cuda.synchronize(dev)
        times["render_ms"] = (time.perf_counter() - t0) * 1e3
    else:
        band = a.band if a.layout == "cyclic" else -(-H // world)
        slot = torch.zeros((D.rows_per_rank(H, world, a.layout, band), W, 3), dtype=torch.uint8, device=dev)   # packed RGB8
        y_first, band_rows, pitch, n_bands = D.band_params(H, world, rank, a.layout, band)
        if n_bands:
            r.render_row_bands(y_first, band_rows, pitch, n_bands, slot, max_depth=a.depth)
        torch.cuda.synchronize(dev)
        times["render_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        gath = torch.empty((world * slot.shape[0], W, 3), dtype=torch.uint8, device=dev)
        dist.all_gather_into_tensor(gath, slot)
        frame = D.assemble(gath, H, world, a.layout, band)
        torch.cuda.synchronize(dev)
        times["gather_assemble_ms"] = (time.perf_counter() - t0) * 1e3
    aa_rays = None
    if a.antialias:
        # the pass reads the QUANTISED frame every rank now holds, so each rank anti-aliases the bands it
        # rendered (no halo exchange) and a second gather of the same shape assembles the result
        t0 = time.perf_counter()
        if world == 1:
            frame, aa_rays = r.antialias(frame, a.aa_threshold, a.aa_level, max_depth=a.depth)
        else:
            def antialias_bands(src, y_first, band_rows, pitch, n_bands, out_slot):
                return r.antialias_row_bands(src, y_first, band_rows, pitch, n_bands, a.aa_threshold, a.aa_level,
                                             max_depth=a.depth, out=out_slot)[1]
            frame, aa_rays = D.antialias_frame_distributed(antialias_bands, frame.contiguous(), H, W, dev, a.layout, band)
        torch.cuda.synchronize(dev)
        times["antialias_ms"] = (time.perf_counter() - t0) * 1e3
    rays = None
    if a.count_rays:
        # the reference's algorithmic counts of the rows this rank rendered; one all-reduce sums the ranks'
        t0 = time.perf_counter()
        names = ("primary", "shadow", "reflect", "refract")
        if world == 1:
            res = r.count_rays(0, H, max_depth=a.depth, pixels=a.ray_map is not None)
            counts = [res[k] for k in names]
        else:
            res = r.count_rays_row_bands(y_first, band_rows, pitch, n_bands, max_depth=a.depth) if n_bands else {}
            sums = torch.tensor([res.get(k, 0) for k in names], dtype=torch.int64, device=dev)
            dist.all_reduce(sums)
            counts = [int(v) for v in sums.tolist()]
        rays = dict(zip(names, counts), total=sum(counts))
        times["count_ms"] = (time.perf_counter() - t0) * 1e3
        if a.ray_map is not None:
            n = res["pixels"].sum(axis=-1, dtype=np.uint64)
            grey = (n * np.uint64(255) // max(n.max(), np.uint64(1))).astype(np.uint8)     # all zero: black
            write_png(a.ray_map, np.ascontiguousarray(np.repeat(grey[..., None], 4, axis=-1)), channels=3)
    hits = None
    if any(getattr(a, flag[2:].replace("-", "_")) is not None for flag in HIT_MAP_FLAGS):
        # first-hit maps (one GPU: the parser refuses the others): one launch, only the planes the maps need
        t0 = time.perf_counter()
        res = r.first_hits(0, H, shadow=a.shadow_map is not None, normal=a.normal_map is not None)
        torch.cuda.synchronize(dev)
        times["first_hits_ms"] = (time.perf_counter() - t0) * 1e3
        planes = {k: v.cpu().numpy() for k, v in res.items()}
        info = scene.info()
        hits = {"objects_hit": int(np.unique(planes["object"][planes["object"] >= 0]).size)}
        for path, grey in hit_maps(a, planes, info["objects"], info["lights"]):
            write_png(path, grey if grey.ndim == 3 else np.repeat(grey[..., None], 4, axis=-1), channels=3)
    paths = None
    if a.ray_paths is not None:
        # the ray debugger's records at the pixel centres of every N-th column and row, row-major (one GPU)
        t0 = time.perf_counter()
        xy = ray_paths_samples(W, H, a.ray_paths_step)
        res = r.ray_paths(xy, max_depth=a.depth)
        paths = {"points": int(xy.shape[0]), "records": int(res["records"].shape[0]),
                 "ms": round((time.perf_counter() - t0) * 1e3, 3)}
        with open(a.ray_paths, "wb") as f:     # (a file object: numpy appends no suffix to the path)
            np.savez(f, xy=xy, offsets=res["offsets"], records=res["records"])
    if rank == 0:
        t0 = time.perf_counter()
        host = frame.cpu().numpy()
        times["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        write_png(a.output, np.ascontiguousarray(host), channels=a.channels)
        times["png_ms"] = (time.perf_counter() - t0) * 1e3
    if world > 1:
        dist.destroy_process_group()
    return {"output": a.output, "width": W, "height": H, "time": a.t, "gpus": world,
            **{k: round(v, 3) for k, v in times.items()}, **({"aa_rays": aa_rays} if a.antialias else {}),
            **({"rays": rays, "rays_per_pixel": round(rays["total"] / (W * H), 3)} if rays is not None else {}),
            **(hits or {}), **({"ray_paths": paths} if paths is not None else {})}


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    a = _parse(argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _self_launch(argv, a.gpus)      # before this process touches the GPU
    info = render(a)
    if int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps(info), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
