"""HIP-event times of the feature pass and of every launch of the a-trous denoiser, on one GPU.

    python tools/post_timing.py [--workload sponza-1080p] [--spp 4] [--reps 20] [--warmup 3] [--out FILE]

Renders one round of the workload at a few samples (the denoiser's input), then times `reps` feature passes and `reps` denoise
calls with the scene's "time_post" switch (rgk_scene_get_post_timing): median, minimum and maximum per launch, beside each
iteration's byte floor -- two 16-byte planes read once and one written, 48 bytes per pixel -- at the card's HBM bandwidth.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TB_S = 8.0  # MI355X HBM3E peak, TB/s (a float4 copy reaches about 6.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import Workload

    wl = Workload(args.workload, scale=args.scale, spp=args.spp)
    scene = rd.Scene(wl.builder.to_desc())

    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    drv = rd.RenderDriver(scene, Cfg, wl.camera)
    drv.render_round()
    dp = drv.default_denoise_params()
    scene.set_tuning(time_post=1)
    P = wl.xres * wl.yres
    aov, dn = [], []
    for r in range(args.warmup + args.reps):
        drv.aov = None
        drv.render_aov()
        t_aov = scene.post_timing(0)
        drv.denoise(dp)
        t_dn = scene.post_timing(1)
        if r >= args.warmup:
            aov.append(t_aov)
            dn.append(t_dn)
    torch.cuda.synchronize()
    lines = [f"{args.workload} {wl.xres}x{wl.yres} ({wl.geometry} geometry), accumulator of {args.spp} spp, {args.reps} repetitions after {args.warmup} warm-up calls; "
             f"HIP events on the scene's stream, ms: median [min .. max]",
             f"denoiser: iterations {dp.iterations}, sigma_color {dp.sigma_color:.4g}, sigma_depth {dp.sigma_depth:.3g}, normal_power_log2 {dp.normal_power_log2}, demodulate {dp.demodulate}"]

    def row(name, xs, floor_bytes=None):
        s = f"  {name:34s} {statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]"
        if floor_bytes:
            floor = floor_bytes / (HBM_TB_S * 1e12) * 1e3
            s += f"   byte floor {floor:.4f} ms ({floor_bytes / 1e6:.1f} MB at {HBM_TB_S:g} TB/s): x{statistics.median(xs) / floor:.2f}"
        return s
    names = ["pixel list + ray generation", "closest-hit walker", "gather (surface point + albedo)"]
    for k, n in enumerate(names):
        lines.append(row("feature pass: " + n, [t[k] for t in aov]))
    lines.append(row("feature pass: all three", [sum(t) for t in aov]))
    it = dp.iterations
    lines.append(row("denoise: prepare", [t[0] for t in dn], P * (12 + 4 + 12 + 12 + 4 + 32)))
    for i in range(it):
        lines.append(row(f"denoise: iteration {i} (step {1 << i})", [t[1 + i] for t in dn], P * 48))
    lines.append(row("denoise: finish", [t[1 + it] for t in dn], P * (16 + 12 + 12)))
    lines.append(row("denoise: whole call", [sum(t) for t in dn]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
