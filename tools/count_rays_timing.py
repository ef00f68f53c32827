"""The ray count (rt_count_rays) against the generic megakernel frame on 4K globes, depth 10 (diagnostic;
DESIGN.md section 6).  Kernel times are rt_ctx_last_kernel_ms (HIP events around the launch), the three launches
alternating in one process after a warm-up; the counts are checked against the CPU oracle's golden totals."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import tinyraytracerinrust_amd as T

S = os.path.join(ROOT, "tests", "golden", "scenes")
W, H, DEPTH, ROUNDS = 3840, 2160, 10, 20
rt = T.RayTracer(W, H)
rt.load_scene(open(os.path.join(S, "globes.scene")).read(), 0.0, asset_dir=S)
r = rt.renderer
r.set_specialize(0, wait=False)                      # the generic megakernel: what bench.py --full reports as such
frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
pixels = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda")
rows = torch.zeros((H, 4), dtype=torch.int64, device="cuda")
launches = {
    "generic frame": lambda: r.render_rows(0, H, max_depth=DEPTH, out=frame),
    "count, totals only": lambda: r.count_rays(0, H, max_depth=DEPTH),
    "count, totals + rows": lambda: r.count_rays(0, H, max_depth=DEPTH, out_rows=rows),
    "count, totals + pixel map": lambda: r.count_rays(0, H, max_depth=DEPTH, out_pixels=pixels),
    "count, rows only": lambda: r.count_rays(0, H, max_depth=DEPTH, out_rows=rows, totals=False),
    "count, pixel map only": lambda: r.count_rays(0, H, max_depth=DEPTH, out_pixels=pixels, totals=False),
}
for _ in range(3):                                   # warm-up: code objects, the frame's tile order
    for f in launches.values():
        f()
torch.cuda.synchronize()
print(r.kernel_info())
ms = {k: [] for k in launches}
for _ in range(ROUNDS):
    for k, f in launches.items():
        res = f()
        torch.cuda.synchronize()
        ms[k].append(r.last_kernel_ms())
base = float(np.mean(ms["generic frame"]))
for k, v in ms.items():
    print(f"{k:28s} mean {np.mean(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({np.mean(v) / base:.3f} x the generic frame)")
res = r.count_rays(0, H, max_depth=DEPTH, out_rows=rows, out_pixels=pixels)
gold = json.load(open(os.path.join(ROOT, "tests", "golden", f"flops_globes_{W}x{H}_t0_d{DEPTH}.json")))["totals"]
want = [gold["ray_primary"], gold["ray_shadow"], gold["ray_reflect"], gold["ray_refract"]]
got = [res[k] for k in ("primary", "shadow", "reflect", "refract")]
px = pixels.cpu().numpy().astype(np.uint64)
print(f"counts {got}  golden {want}  equal {got == want}; pixel map sums {px.sum(axis=(0, 1)).tolist()}, "
      f"row sums {rows.cpu().numpy().sum(axis=0).tolist()}; most rays on a pixel {int(px.sum(axis=-1).max())}; "
      f"rays per pixel {res['total'] / (W * H):.3f}")
sys.exit(0 if got == want and px.sum(axis=(0, 1)).tolist() == want else 1)
