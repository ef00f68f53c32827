"""Load / wait listing of the scene-specialised kernels' assembly (csrc/spec_text.cpp): compiles a scene's
program offline as tools/spec_resources.py does, with -S, and prints per kernel its resource line and
every scalar load, global (vector) load and s_waitcnt of the function body with its line number in the
body -- the yardstick of the prologue, light-loop and epilogue memory trips (DESIGN.md "Dispatch records").
Scratch (spill) traffic is counted, not listed.

  python3 tools/spec_asm_loads.py globes 3840 2160 /tmp/spec_asm 'rows_00|prim_00' > profiles/NAME.txt
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
os.environ.setdefault("RT_NO_TORCH_PRELOAD", "1")

LISTED = re.compile(r"^\s+(s_load_\w+|s_buffer_load_\w+|global_load_\w+|flat_load_\w+|s_waitcnt)\b")
CLASSES = [("scalar loads", r"^\s+s_(buffer_)?load_"), ("global loads", r"^\s+(global|flat)_load_"),
           ("scratch loads", r"^\s+scratch_load_"), ("scratch stores", r"^\s+scratch_st"), ("s_waitcnt", r"^\s+s_waitcnt\b"),
           ("v_readfirstlane", r"^\s+v_readfirstlane_b32"), ("s_cselect", r"^\s+s_cselect_")]


def main():
    import tinyraytracerinrust_amd as T
    from tests.conftest import SCENES, scene_text
    name = sys.argv[1] if len(sys.argv) > 1 else "globes"
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 3840
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 2160
    out = sys.argv[4] if len(sys.argv) > 4 else "/tmp/spec_asm"
    only = sys.argv[5] if len(sys.argv) > 5 else "rows_00|prim_00"
    os.makedirs(out, exist_ok=True)
    text = (T.Scene.compile(scene_text(name), 0.0, W, H, asset_dir=SCENES) if name != "sphere" else
            T.Scene.compile("draw(sphere(<0, 0, 0>, 30, red))", 0.0, W, H)).spec_program()
    cut = text.index('extern "C" __global__')
    prelude, kernels = text[:cut], text[cut:]
    csrc = os.path.join(ROOT, "tinyraytracerinrust_amd", "csrc")
    for k in re.split(r'(?=extern "C" __global__)', kernels):
        if not k.strip():
            continue
        kname = re.search(r"void (rt_spec_\w+)\(", k).group(1)
        if only and not re.search(only, kname):
            continue
        label = kname
        src, asm = os.path.join(out, kname + ".hip"), os.path.join(out, kname + ".s")
        if os.environ.get("NM"):           # the mask-free megakernel (spec_text.cpp SPEC_ROWS_NOMASK): RT_TILE_MASKS 0, a null table
            kname += "_nm"
            k = "#define RT_TILE_MASKS 0\n" + k.replace("s_frames, masks", "s_frames, nullptr")
            src, asm = os.path.join(out, kname + ".hip"), os.path.join(out, kname + ".s")
            with open(src, "w") as f:
                f.write(k[:k.index("extern")] + prelude + k[k.index("extern"):])
        else:
            with open(src, "w") as f:
                f.write(prelude + k)
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
               "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-S", "-o", asm, src,
               "-Rpass-analysis=kernel-resource-usage", "-I", csrc]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            print(r.stderr[-3000:])
            raise SystemExit(f"{kname}: compile failed")
        rem = dict(re.findall(r"remark:\s+(.+?):\s*(\S+)\s*\[-Rpass", r.stderr))
        keys = ["VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]
        lines = open(asm).read().split("\n")
        b = next(i for i, l in enumerate(lines) if l.startswith(label + ":"))
        e = next(i for i in range(b, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l for l in lines[b + 1:e] if l.strip() and not l.lstrip().startswith((";", "."))]
        print(f"== {kname} ({name} {W}x{H}): " + " ".join(f"{k}={rem.get(k, '?')}" for k in keys))
        print(f"   {len(body)} instructions and labels; " +
              ", ".join(f"{sum(1 for l in body if re.search(p, l))} {n}" for n, p in CLASSES))
        for i, l in enumerate(body, 1):
            if LISTED.search(l):
                print(f"{i:6d} {l.strip()}")


if __name__ == "__main__":
    main()
