"""What the tile-mask predicate (csrc/rt_tilemask.h) leaves for the row kernels to walk, evaluated on the
host (rt_scene_tile_masks, no GPU): per config the share of walks whose word holds no boxed object, the boxed
bits set per walk, and the same per class.  A walk is a tile's primary walk, and on a floor tile (its shadow
words were computed) one shadow walk per light and the reflection walk.  RT_LIB_PATH picks another build.
usage: python tools/mask_stats.py [globes4k globes1080 ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = os.path.join(ROOT, "tests", "golden", "scenes")
CONFIGS = {"globes4k": ("globes", 3840, 2160), "globes1080": ("globes", 1920, 1080), "globes96": ("globes", 96, 72),
           "three_cubes1080": ("three_cubes", 1920, 1080), "ground_star1080": ("ground_star", 1920, 1080)}
ONES = 0xFFFFFFFF


def stats(name):
    import tinyraytracerinrust_amd as T
    scene, W, H = CONFIGS[name]
    sc = T.Scene.compile(open(os.path.join(S, scene + ".scene")).read(), 0.0, W, H, asset_dir=S)
    words, info = sc.tile_masks()
    boxed = np.uint32(info["boxed"])
    n_lights = sc.info()["lights"]
    pop = lambda w: np.array([bin(int(v)).count("1") for v in np.unique(w)])[np.unique(w, return_inverse=True)[1]]
    floor = words[:, 1] != ONES
    prim = words[:, 0] & boxed
    cls = {"prim": prim}
    for l in range(min(n_lights, 4)):
        cls[f"shadow[{l}]"] = words[floor, 1 + l] & boxed
    cls["refl"] = words[floor, 5] & boxed
    allw = np.concatenate(list(cls.values()))
    print(f"{name}: {len(words)} tiles, {floor.sum()} floor tiles, {len(allw)} walks; boxed {int(boxed):#x}")
    print(f"  provably empty walks {100.0 * np.mean(allw == 0):.1f} %, boxed bits set per walk {pop(allw).mean():.3f}")
    for k, w in cls.items():
        print(f"  {k:10s} mean bits {pop(w).mean():.3f}, empty {100.0 * np.mean(w == 0):.1f} %")
    sky = words[:, 0] == 0
    four = floor & ((words[:, 0] & boxed) == 0) & ((words[:, 5] & boxed) == 0)
    for l in range(min(n_lights, 4)):
        four &= (words[:, 1 + l] & boxed) == 0
    print(f"  sky tiles {100.0 * sky.mean():.1f} %, floor tiles with every word empty {100.0 * four.sum() / max(1, floor.sum()):.1f} %")
    n_obj = sc.info()["objects"]
    for l in range(min(n_lights, 4)):
        per = [100.0 * np.mean((words[floor, 1 + l] >> o) & 1) for o in range(n_obj)]
        print(f"  shadow[{l}] per object, % of floor tiles: " + " ".join(f"{p:.0f}" for p in per))


if __name__ == "__main__":
    for n in sys.argv[1:] or ["globes4k", "globes1080"]:
        stats(n)
