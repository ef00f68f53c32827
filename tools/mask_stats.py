"""What the tile-mask predicate (csrc/rt_tilemask.h) leaves for the row kernels to walk, evaluated on the
host (rt_scene_tile_masks, no GPU): per config the share of walks whose word holds no boxed object, the boxed
bits set per walk, and the same per class.  A walk is a tile's primary walk, and on a floor tile (its shadow
words were computed) one shadow walk per light and the reflection walk.  RT_LIB_PATH picks another build.
usage: python tools/mask_stats.py [--truth] [globes4k globes1080 ...]
--truth: the predicate's classes against the pixel centres' own rays in the CPU oracle (minutes per 4K frame)."""
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


def truth(name):
    """--truth: the predicate's classes against what the pixel centres' own rays do, from the CPU oracle alone
    (orc_hit_signature per pixel: the object hit and the occluded lights; record_rays on floor pixels: the depth-1
    ray's hit) -- the bound on what a table traced per entry (RT_OPT_TRACED_MASKS) can reclassify.  And the object
    tiles (a pixel on a boxed object; RT_OPT_TRACED_MASKS 1 / 3 trace them too, with every pixel that hits anything):
    those with no occluded pixel per light and for every light, the objects their depth-1 rays hit, and those whose
    pixels spawn no depth-1 ray -- the bound the device's words of flagged entries are compared with."""
    import tinyraytracerinrust_amd as T
    from oracle import oracle as O
    scene, W, H = CONFIGS[name]
    text = open(os.path.join(S, scene + ".scene")).read()
    O.register_texture_file("worldmap.png", os.path.join(S, "worldmap.png"))
    sc = T.Scene.compile(text, 0.0, W, H, asset_dir=S)
    words, info = sc.tile_masks()
    boxed, plane = np.uint32(info["boxed"]), info["plane"]
    orc = O.OracleScene(text, 0.0, W, H, max_depth=2)
    n_lights = min(orc.n_lights, 4)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    obj = np.zeros(tx * ty, bool)                    # the tile holds a pixel on a boxed object
    hit = np.zeros(tx * ty, bool)                    # ... a pixel that hits anything
    occl = np.zeros((n_lights, tx * ty), bool)       # ... a floor pixel whose light l is occluded
    refl = np.zeros(tx * ty, bool)                   # ... a floor pixel whose depth-1 ray hits
    o_occl = np.zeros((n_lights, tx * ty), bool)     # ... a pixel, floor or object, whose light l is occluded
    o_refl = np.zeros(tx * ty, np.uint32)            # the objects hit by the depth-1 rays of the tile's pixels
    o_spawn = np.zeros(tx * ty, bool)                # ... a pixel that spawns a depth-1 ray
    for y in range(H):
        for x in range(W):
            sig = orc.hit_signature(x, y)
            if sig < 0:
                continue
            t = (y // 8) * tx + x // 8
            hit[t] = True
            for l in range(n_lights):
                if (sig // 4096 >> l) & 1:
                    o_occl[l, t] = True
            if sig % 4096 - 1 != plane:
                obj[t] = True
                continue
            for l in range(n_lights):
                if (sig // 4096 >> l) & 1:
                    occl[l, t] = True
            if not refl[t]:
                r = orc.record_rays(x, y, cap=4)[0].view(T.RAY_RECORD_DTYPE)
                refl[t] = bool(((r["depth"] == 1) & (r["intersected"] != 0)).any())
    floor_t = hit & ~obj                             # every hit of the tile is on the floor
    for t in np.flatnonzero(obj):                    # the object tiles' depth-1 rays, every pixel that hits anything
        for y in range((t // tx) * 8, min((t // tx) * 8 + 8, H)):
            for x in range((t % tx) * 8, min((t % tx) * 8 + 8, W)):
                if orc.hit_signature(x, y) < 0:
                    continue
                r = orc.record_rays(x, y, cap=4)[0].view(T.RAY_RECORD_DTYPE)
                d1 = r[r["depth"] == 1]
                if len(d1):
                    o_spawn[t] = True
                    if d1[0]["intersected"]:
                        o_refl[t] |= np.uint32(1) << np.uint32(d1[0]["object"])
    p_sky = words[:, 0] == 0
    p_prim = (words[:, 0] & boxed) != 0
    p_floor = ~p_sky & ~p_prim
    print(f"{name} --truth: {tx * ty} tiles; class: predicate | oracle, pixel centres")
    print(f"  sky tiles: {p_sky.sum()} | {(~hit).sum()} (every primary ray misses)")
    print(f"  tiles with a boxed bit in prim: {p_prim.sum()} | {obj.sum()} hold an object pixel; of the predicate's "
          f"{(p_prim & floor_t).sum()} are all floor, {(p_prim & ~hit).sum()} all sky")
    for l in range(n_lights):
        p_sh = p_floor & ((words[:, 1 + l] & boxed) != 0)
        print(f"  floor tiles with a boxed bit in shadow[{l}]: {p_sh.sum()} | {(floor_t & occl[l]).sum()} all-floor tiles have an "
              f"occluded pixel; the word is set with no occluded pixel on {(p_sh & floor_t & ~occl[l]).sum()} all-floor tiles")
    p_lean = p_floor & ((words[:, 5] & boxed) == 0)
    for l in range(n_lights):
        p_lean &= (words[:, 1 + l] & boxed) == 0
    unshadowed = floor_t & ~occl.any(axis=0)
    print(f"  lean tiles (predicate candidates): {p_lean.sum()} | {(unshadowed & ~refl).sum()} are all floor, unshadowed and no "
          f"depth-1 ray hits; {unshadowed.sum()} are all floor and unshadowed, {(unshadowed & ((words[:, 5] & boxed) != 0)).sum()} of "
          f"those have a boxed bit in refl")
    n_obj = int(obj.sum())
    print(f"  object tiles: {n_obj}; no pixel occluded: " +
          ", ".join(f"light {l} {(obj & ~o_occl[l]).sum()} ({100.0 * (obj & ~o_occl[l]).sum() / max(1, n_obj):.0f} %)" for l in range(n_lights)) +
          f", every light {(obj & ~o_occl.any(axis=0)).sum()} ({100.0 * (obj & ~o_occl.any(axis=0)).sum() / max(1, n_obj):.0f} %)")
    bits = np.array([bin(int(v)).count("1") for v in o_refl[obj]])
    print(f"  object tiles: objects hit by depth-1 rays, mean per tile {bits.mean() if n_obj else 0.0:.3f} (the plane included); "
          f"every pixel spawns no depth-1 ray on {(obj & ~o_spawn).sum()} tiles")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--truth"]
    for n in args or ["globes4k", "globes1080"]:
        (truth if "--truth" in sys.argv[1:] else stats)(n)
