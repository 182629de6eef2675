"""HIP-event times of the guided upsampler's two launches, on one GPU.

    python tools/upsample_timing.py [--workload sponza-1080p] [--spp 4] [--reps 20] [--warmup 3] [--out FILE]

Renders one round of the workload at a quarter of its size on each axis (what -p does), then times `reps` calls of
RenderDriver.upsample to the full size with the scene's "time_post" switch (rgk_scene_get_post_timing 7), and the feature pass of
the full grid (0) that the first call pays once: median, minimum and maximum per launch.  Beside each kernel the bytes it has to
move at least once -- every input and output plane once, the record planes once per kernel -- and the time that takes at the
card's HBM bandwidth.
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
    W, H = wl.xres, wl.yres
    WL, HL = W // 4, H // 4
    wl.cfg.xres, wl.cfg.yres = WL, HL
    low_cam = wl.cfg.get_camera()
    wl.cfg.xres, wl.cfg.yres = W, H
    scene = rd.Scene(wl.builder.to_desc())
    prm = wl.params()
    prm.xres, prm.yres = WL, HL

    class Cfg:
        xres, yres, render_rounds, render_minutes = WL, HL, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: prm)
    drv = rd.RenderDriver(scene, Cfg, low_cam)
    drv.render_round()
    drv.render_aov()
    scene.set_tuning(time_post=1)
    up = drv.default_upsample_params()
    us, aov, shares = [], [], None
    for r in range(args.warmup + args.reps):
        drv._up_key = None  # the full grid's feature pass again
        _, sup = drv.upsample(wl.camera, W, H, up)
        t_aov, t_us = scene.post_timing(0), scene.post_timing(7)
        if r >= args.warmup:
            us.append(t_us)
            aov.append(t_aov)
        shares = [float((sup == k).double().mean()) for k in (0, 1, 2)]
    torch.cuda.synchronize()
    P, Pl = W * H, WL * HL
    lines = [f"{args.workload} {W}x{H} from {WL}x{HL} ({wl.geometry} geometry), low accumulator of {args.spp} spp, {args.reps} repetitions after {args.warmup} warm-up calls; "
             f"HIP events on the scene's stream, ms: median [min .. max]",
             f"upsampler: plane_tol {up.plane_tol:.3g}, normal_cos {up.normal_cos:.3g}, demodulate {up.demodulate}, albedo_floor {up.albedo_floor:.3g}; "
             f"support 0 / 1 / 2 shares {shares[0]:.4f} / {shares[1]:.4f} / {shares[2]:.4f}"]

    def row(name, xs, floor_bytes=None):
        s = f"  {name:40s} {statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]"
        if floor_bytes:
            floor = floor_bytes / (HBM_TB_S * 1e12) * 1e3
            s += f"   byte floor {floor:.4f} ms ({floor_bytes / 1e6:.2f} MB at {HBM_TB_S:g} TB/s): x{statistics.median(xs) / floor:.1f}"
        return s
    alb = 12 if up.demodulate else 0  # the albedo planes are read only to divide and multiply
    # prepare: accumulator 12 + 4, [albedo 12,] normal 12, depth 4 read, three 16-byte records written, per low pixel
    lines.append(row("k_us_prepare", [t[0] for t in us], Pl * (32 + alb + 48)))
    # gather: [albedo 12,] normal 12, depth 4 read, 12 + 1 written per full pixel; the record planes read once
    lines.append(row("k_us_gather", [t[1] for t in us], P * (16 + alb + 13) + Pl * 48))
    lines.append(row("upsample: both launches", [sum(t) for t in us]))
    for k, n in enumerate(["pixel list + ray generation", "closest-hit walker", "gather (surface point + albedo)"]):
        lines.append(row("full-grid feature pass: " + n, [t[k] for t in aov]))
    lines.append(row("full-grid feature pass: all three", [sum(t) for t in aov]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
