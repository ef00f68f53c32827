"""One rank's share of the anti-aliasing pass at N ranks, emulated on one GPU (diagnostic; tools/aa_timing.py's
sibling, measured the way tools/rank_share_probe.py measures a rank's render share).

The 4K globes frame (threshold 0.01, level 3) with the scene's specialised sample kernels loaded: the whole-frame
pass (rt_antialias), then for N = 2, 4, 8 every rank's cyclic 8-row bands (rt_antialias_row_bands with
distributed.band_params) on the one context: wall time with a device synchronisation and the pass' kernel span
(rt_ctx_last_kernel_ms), medians over --rounds; the ranks' rays must sum to the whole frame's and their rows,
assembled, must be its bytes.
usage: python tools/aa_band_share.py [--rounds 9] [--size 3840x2160] [--band 8]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--band", type=int, default=8)
    a = ap.parse_args()
    import torch
    import tinyraytracerinrust_amd as T
    from tinyraytracerinrust_amd import distributed as D
    W, H = (int(v) for v in a.size.split("x"))
    th, level = 0.01, 3
    sc = T.Scene.compile(open(os.path.join(S, "globes.scene")).read(), 0.0, W, H, asset_dir=S)
    r = T.Renderer(0, specialize=1)
    r.upload(sc)
    assert r.spec_wait(-1) and r.spec_wait_samples(-1)
    frame = r.render_rows(0, H)
    frame = r.render_rows(0, H, out=frame)
    torch.cuda.synchronize()

    def timed(fn):
        fn()                                                   # warm-up (the first pass allocates)
        torch.cuda.synchronize()
        wall, kern = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(r.last_kernel_ms())
        return statistics.median(wall), min(wall), max(wall), statistics.median(kern)

    whole = torch.empty_like(frame)
    rays = [0]

    def pass_whole():
        rays[0] = r.antialias(frame, th, level, out=whole)[1]
    w = timed(pass_whole)
    print(f"globes {W}x{H} threshold {th} level {level}: {rays[0]} sub-pixel rays; {r.sample_kernel_info()}")
    print(f"whole frame (rt_antialias): {w[0]:.3f} ms wall ({w[1]:.3f}-{w[2]:.3f}), kernel span {w[3]:.3f} ms", flush=True)
    for n in (2, 4, 8):
        slot_rows = D.rows_per_rank(H, n, "cyclic", a.band)
        slots = torch.zeros((n * slot_rows, W, 4), dtype=torch.uint8, device=frame.device)
        res, total = [], 0
        for rank in range(n):
            params = D.band_params(H, n, rank, "cyclic", a.band)
            slot = slots[rank * slot_rows:(rank + 1) * slot_rows]
            got = [0]

            def pass_bands():
                got[0] = r.antialias_row_bands(frame, *params, th, level, out=slot)[1]
            res.append(timed(pass_bands))
            total += got[0]
        assert total == rays[0], (total, rays[0])
        assert torch.equal(D.assemble(slots, H, n, "cyclic", a.band), whole), "band rows differ from the whole frame's"
        med = [x[0] for x in res]
        print(f"N={n}: cyclic {a.band}-row bands, {slot_rows} rows per rank: rank 0 {med[0]:.3f} ms wall "
              f"({res[0][1]:.3f}-{res[0][2]:.3f}), kernel span {res[0][3]:.3f} ms; ranks' medians {min(med):.3f}-{max(med):.3f} ms wall "
              f"= {100 * max(med) / w[0]:.0f} % of the whole-frame pass (1/N = {100 / n:.1f} %); same bytes, rays sum to the whole frame's",
              flush=True)


if __name__ == "__main__":
    main()
