"""HIP-event times of the variance-guided filter and of the noise estimate beside the fixed-sigma denoiser, on one GPU.

    python tools/noise_timing.py [--workload sponza-1080p] [--spp 2] [--reps 20] [--warmup 3] [--out FILE]

Renders two rounds of the workload with noise tracking (the halves), then alternates rgk_denoise_device,
rgk_denoise_variance_device and rgk_noise_estimate_device in one process, `reps` times after `warmup` calls, with the scene's
"time_post" switch (rgk_scene_get_post_timing 1 / 2 / 3): median, minimum and maximum per launch, and the ratio of the two
filters' whole calls.  The baseline is the fixed filter of the same run, not a figure from another day.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tile-size", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rgk_amd import capi, render_driver as rd
    from rgk_amd.workloads import Workload

    wl = Workload(args.workload, scale=args.scale, spp=args.spp)
    scene = rd.Scene(wl.builder.to_desc())

    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 2, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    drv = rd.RenderDriver(scene, Cfg, wl.camera, track_noise=True)
    drv.render_round()
    drv.render_round()
    dp, vp = drv.default_denoise_params(), capi.DenoiseVarParams()
    scene.set_tuning(time_post=1)
    fixed, guided, sums = [], [], []
    for r in range(args.warmup + args.reps):
        drv.denoise(dp)
        t1 = scene.post_timing(1)
        drv.denoise_variance(vp)
        t2 = scene.post_timing(2)
        nz = drv.noise(args.tile_size)
        t3 = scene.post_timing(3)
        if r >= args.warmup:
            fixed.append(t1)
            guided.append(t2)
            sums.append(t3)
    torch.cuda.synchronize()
    lines = [f"{args.workload} {wl.xres}x{wl.yres} ({wl.geometry} geometry), accumulator of 2 x {args.spp} spp, relative noise {nz['rel']:.4f}; {args.reps} repetitions after "
             f"{args.warmup} warm-up calls, the three entries alternating in one process; HIP events on the scene's stream, ms: median [min .. max]",
             f"fixed filter: iterations {dp.iterations}, sigma_color {dp.sigma_color:.4g}; variance-guided: iterations {vp.iterations}, sigma_k {vp.sigma_k:g}, "
             f"albedo_floor {vp.albedo_floor:g}; both sigma_depth {vp.sigma_depth:.3g}, normal_power_log2 {vp.normal_power_log2}, demodulate {vp.demodulate}"]

    def row(name, xs):
        return f"  {name:44s} {statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]"
    it = dp.iterations
    lines.append(row("fixed: prepare", [t[0] for t in fixed]))
    for i in range(it):
        lines.append(row(f"fixed: iteration {i} (step {1 << i})", [t[1 + i] for t in fixed]))
    lines.append(row("fixed: finish", [t[1 + it] for t in fixed]))
    lines.append(row("fixed: whole call", [sum(t) for t in fixed]))
    it = vp.iterations
    lines.append(row("variance-guided: prepare", [t[0] for t in guided]))
    lines.append(row("variance-guided: prefilter (5 x 5, step 1)", [t[1] for t in guided]))
    for i in range(it):
        lines.append(row(f"variance-guided: iteration {i} (step {1 << i})", [t[2 + i] for t in guided]))
    lines.append(row("variance-guided: finish", [t[2 + it] for t in guided]))
    lines.append(row("variance-guided: variance copy", [t[3 + it] for t in guided]))
    lines.append(row("variance-guided: whole call", [sum(t) for t in guided]))
    ratios = [sum(g) / sum(f) for g, f in zip(guided, fixed)]
    lines.append(f"  variance-guided / fixed, whole calls, per repetition: {statistics.median(ratios):.3f}  [{min(ratios):.3f} .. {max(ratios):.3f}]")
    lines.append(row(f"noise estimate: tile sums (tile_size {args.tile_size}, {nz['tiles'].size} tiles)", [t[0] for t in sums]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
