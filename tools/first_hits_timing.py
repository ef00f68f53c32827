"""The first-hit maps (rt_first_hits) against the generic megakernel frame on 4K globes, at depth 0 and depth 10
(diagnostic).  Kernel times are rt_ctx_last_kernel_ms (HIP events around the launch), the
launches alternating in one process after a warm-up, RT_OPT_SPECIALIZE 0; the maps are checked against the ray
count's pixel map (a pixel casts shadow rays exactly where it has a first hit) and against each other."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import tinyraytracerinrust_amd as T

S = os.path.join(ROOT, "tests", "golden", "scenes")
W, H, ROUNDS = 3840, 2160, 20
rt = T.RayTracer(W, H)
rt.load_scene(open(os.path.join(S, "globes.scene")).read(), 0.0, asset_dir=S)
r = rt.renderer
r.set_specialize(0, wait=False)                      # the generic megakernel: what bench.py --full reports as such
frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
planes = {"object": torch.empty((H, W), dtype=torch.int32, device="cuda"),
          "distance": torch.empty((H, W), dtype=torch.float64, device="cuda"),
          "shadow": torch.empty((H, W), dtype=torch.uint32, device="cuda"),
          "normal": torch.empty((H, W, 3), dtype=torch.float64, device="cuda")}


def hits(*names):
    return lambda: r.first_hits(0, H, out={k: planes[k] for k in ("object", "distance") + names})


launches = {
    "generic frame, depth 0": lambda: r.render_rows(0, H, max_depth=0, out=frame),
    "generic frame, depth 10": lambda: r.render_rows(0, H, max_depth=10, out=frame),
    "first hits, id + distance": hits(),
    "first hits, + normal": hits("normal"),
    "first hits, + shadow": hits("shadow"),
    "first hits, every plane": hits("shadow", "normal"),
}
for _ in range(3):                                   # warm-up: code objects, the frames' tile orders
    for f in launches.values():
        f()
torch.cuda.synchronize()
print(r.kernel_info())
ms = {k: [] for k in launches}
for _ in range(ROUNDS):
    for k, f in launches.items():
        f()
        torch.cuda.synchronize()
        ms[k].append(r.last_kernel_ms())
base = float(np.mean(ms["generic frame, depth 0"]))
for k, v in ms.items():
    print(f"{k:28s} mean {np.mean(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({np.mean(v) / base:.3f} x the depth-0 frame)")
# the maps: a depth-0 pixel casts its lights' shadow rays exactly where it has a first hit
counts = r.count_rays(0, H, max_depth=0, pixels=True)
res = hits("shadow", "normal")()
torch.cuda.synchronize()
obj = res["object"].cpu().numpy()
dist = res["distance"].cpu().numpy()
shadow = res["shadow"].view(torch.int32).cpu().numpy()
hit = obj >= 0
n_lights = rt.scene.info()["lights"]
ok = (np.array_equal(counts["pixels"][..., 1] == n_lights, hit) and np.isposinf(dist[~hit]).all()
      and np.isfinite(dist[hit]).all() and (shadow[~hit] == 0).all() and int(obj.max()) < rt.scene.info()["objects"])
print(f"hit share {hit.mean():.4f}, objects visible {np.unique(obj[hit]).size}, shadowed share of hits "
      f"{(shadow[hit] != 0).mean():.4f}, nearest {dist[hit].min():.3f}, farthest {dist[hit].max():.3f}; "
      f"hits equal the ray count's shaded pixels and misses are (-1, inf, 0): {ok}")
sys.exit(0 if ok else 1)
