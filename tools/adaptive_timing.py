"""Adaptive tile sampling on one GPU: what the round fold costs beside the whole-frame additions it replaces, and what a frame
rendered to a fixed noise level costs with and without it.

    python tools/adaptive_timing.py [--workload sponza-1080p] [--spp 4] [--reps 20] [--warmup 3] [--rounds 32] [--min-visits 4] [--out FILE]

1. The fold.  Done in torch, a tracked round clears the per-round accumulator (two whole-frame fills) and adds it to the total
   (two additions) and, on odd rounds, to the half-buffer (two more).  Those torch calls, between two events on torch's stream, are
   the baseline; rgk_round_fold_device over every tile of the frame, with the scene's "time_post" switch (rgk_scene_get_post_timing
   4: the copy of the tile list, the fold), is what stands in for them.  The two alternate in one process, `reps` times after
   `warmup`, on scratch accumulators of the frame's size; a fold of every tenth tile is timed beside them.
2. The frame.  X = the uniform tracked driver's estimate after `rounds` rounds; then a uniform frame and an adaptive frame, each to
   until_noise = X and at most 4 x `rounds` rounds: rounds, paths (sum of counters[].paths), wall time around render_frame, and the
   adaptive frame's live tiles per round.  The baseline is the uniform frame of the same run.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--min-visits", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rgk_amd import capi, render_driver as rd
    from rgk_amd.workloads import Workload

    wl = Workload(args.workload, scale=args.scale, spp=args.spp)
    scene = rd.Scene(wl.builder.to_desc())
    dev = torch.device("cuda", scene.device)
    W, H = wl.xres, wl.yres

    class Cfg:
        xres, yres, render_rounds, render_minutes = W, H, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    lines = [f"{args.workload} {W}x{H} ({wl.geometry} geometry), {args.spp} spp per round"]

    # ---- 1. the fold against the torch calls it replaces
    tiles = rd.generate_task_list(W, H)
    tenth = (capi.Tile * len(range(0, len(tiles), 10)))(*[tiles[i] for i in range(0, len(tiles), 10)])
    rnd, tot, half = (rd.EXRTexture(W, H, dev) for _ in range(3))
    rnd.data.uniform_(0.0, 1.0)
    ptrs = [t.data_ptr() for t in (rnd.data, rnd.count, tot.data, tot.count, half.data, half.count)]

    def torch_ms(odd):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rnd.data.zero_()
        rnd.count.zero_()
        for dst in (tot, half) if odd else (tot,):
            dst.data += rnd.data
            dst.count += rnd.count
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def fold_ms(tl, odd):
        torch.cuda.synchronize()
        scene.round_fold_device(W, H, tl, np.full(len(tl), 1 if odd else 0, np.uint8), *ptrs)
        return scene.post_timing(4)
    scene.set_tuning(time_post=1)
    got = {k: [] for k in ("torch even", "torch odd", "fold even", "fold odd", "fold odd, every tenth tile")}
    for r in range(args.warmup + args.reps):
        ms = {"torch even": torch_ms(False), "fold even": fold_ms(tiles, False), "torch odd": torch_ms(True), "fold odd": fold_ms(tiles, True),
              "fold odd, every tenth tile": fold_ms(tenth, True)}
        if r >= args.warmup:
            for k, v in ms.items():
                got[k].append(v)
    scene.set_tuning(time_post=0)
    P = W * H
    lines.append(f"1. round fold, {len(tiles)} tiles ({len(tenth)} in the sparse list); {args.reps} repetitions after {args.warmup} warm-up calls, alternating in one "
                 "process; ms: median [min .. max].  Baseline: the torch fills and additions of a tracked driver's round, events on torch's stream")

    def row(name, xs, note=""):
        return f"  {name:52s} {statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]{note}"
    for parity, planes in (("even", 2), ("odd", 3)):
        # bytes the fold needs: per pixel 16 B (rgb + count) read from each of `planes` buffers and written to each
        gbs = 2 * planes * 16 * P / (statistics.median([t[1] for t in got[f"fold {parity}"]]) * 1e-3) / 1e9
        lines.append(row(f"torch, {parity} round: 2 fills + {2 * (planes - 1)} additions", got[f"torch {parity}"]))
        lines.append(row(f"fold, {parity} round: copy of the tile list", [t[0] for t in got[f"fold {parity}"]]))
        lines.append(row(f"fold, {parity} round: k_round_fold", [t[1] for t in got[f"fold {parity}"]], f"   {gbs:.0f} GB/s of the {2 * planes * 16} B per pixel it must move"))
    lines.append(row("fold, odd round, every tenth tile: copy", [t[0] for t in got["fold odd, every tenth tile"]]))
    lines.append(row("fold, odd round, every tenth tile: k_round_fold", [t[1] for t in got["fold odd, every tenth tile"]]))

    # ---- 2. a frame to a fixed noise level
    probe = rd.RenderDriver(scene, Cfg, wl.camera, track_noise=True)
    for _ in range(args.rounds):
        probe.render_round()
    X = probe.noise()["rel"]
    lines.append(f"2. frames to until_noise = {X:.5f} (the uniform estimate after {args.rounds} rounds), at most {4 * args.rounds} rounds, min_visits {args.min_visits}.  "
                 "Baseline: the uniform frame of this run")
    for name in ("uniform", "adaptive", "uniform again"):
        live = []
        drv = rd.RenderDriver(scene, Cfg, wl.camera, track_noise=True, adaptive=capi.AdaptParams(min_visits=args.min_visits) if name == "adaptive" else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.render_frame(rounds=4 * args.rounds, until_noise=X, on_noise=(lambda r, rel, n: live.append(n)) if name == "adaptive" else None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        paths = sum(int(c.paths) for c in drv.counters)
        lines.append(f"  {name:14s} rounds {drv.rounds_done:4d}  paths {paths:13d}  wall {dt:8.3f} s  relative noise {drv.noise()['rel']:.5f}")
        if live:
            lines.append(f"  {'':14s} live tiles of {drv.n_tasks} after rounds 2..: " + " ".join(str(n) for n in live))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
