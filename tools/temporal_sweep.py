"""Temporal reuse measured on one GPU: the parameter sweep behind the shipped capi.TemporalParams, and the kernel times.

    python tools/temporal_sweep.py [--frames 16] [--spp 4] [--ref-spp 1024] [--size 96] [--out FILE]

1. Cornell with spheres (tests/golden), `frames` consecutive frames of the -r animation (t = k / 500) at `spp` samples each.  Every
   frame is rendered once; each parameter set then runs the chain reproject -> blend -> filter over the same accumulators.
   Reported per set: relative L2 of a frame's temporal image against a `ref-spp` render of the same camera over the pixels
   whose first hit is not specular -- the mean over the second half of the chain (what a set is chosen by), the last frame, and
   the third frame (what tests/test_gpu_temporal.py gates) -- and the share of a frame's pixels that found history.  The single-frame denoise() of the same frames is the line to beat.
   One parameter moves at a time from the starting values of the issue (plane_tol 0.01, normal_cos 0.9, alpha_min 0.1,
   max_len 10, albedo_floor 0.02), then the best of each is combined.
2. rgk_temporal_reproject_device / rgk_temporal_blend_device at 1920 x 1080 on the Sponza workload's feature planes of two
   cameras of its animation, with the scene's "time_post" switch (rgk_scene_get_post_timing 5): median [min .. max] of `reps` calls.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rgk_amd import capi, render_driver as rd
    from rgk_amd.config import make_camera
    from rgk_amd.scene import glm_rotate
    from rgk_amd.workloads import SceneFixture, Workload
    import temporal_ref as T

    F = np.float32
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rel_l2(a, b):
        return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))

    def turned(c, t, W, H):
        pos, lookat, up = (np.array(c[k], F) for k in ("pos", "lookat", "up"))
        if t != 0.0:
            rot = glm_rotate(F(t) * F(2.0) * F(math.pi), up)[:3, :3]
            pos = lookat - (rot @ (lookat - pos)).astype(F)
        return make_camera(pos, lookat, up, fov=c.get("fov"), focal=c.get("focal"), xres=W, yres=H)

    # ---- 1. the sweep
    W = H = args.size
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_cornell-box-spheres.npz"), spp=args.spp)
    desc = wl.builder.to_desc()
    scene = rd.Scene(desc)

    def cfg(spp):
        prm = wl.params()
        prm.xres, prm.yres, prm.multisample = W, H, spp

        class Cfg:
            xres, yres, render_rounds, render_minutes = W, H, 1, None
            get_params = staticmethod(lambda sampler=0, flags=0: prm)
        return Cfg
    cams = [turned(wl.builder.extra["camera"], k / 500.0, W, H) for k in range(args.frames)]
    drivers = []
    for cam in cams:
        d = rd.RenderDriver(scene, cfg(args.spp), cam, history=rd.TemporalHistory())
        d.render_round()
        d.render_aov()
        drivers.append(d)
    kinds = T.tri_kinds(desc)
    refs, keeps = {}, {}
    half = list(range(args.frames // 2, args.frames))  # the frames a parameter set is scored on: the chain has its full length there
    for k in sorted({2, *half}):
        r = rd.RenderDriver(scene, cfg(args.ref_spp), cams[k])
        r.render_round()
        refs[k] = r.total_ob.get_pixels().cpu().numpy()
        tri = r.render_aov()["tri"].cpu().numpy()
        keeps[k] = ~((tri >= 0) & np.isin(kinds[np.where(tri >= 0, tri, 0)], T.SPECULAR_KINDS))

    def err(img, k):
        return rel_l2(img.cpu().numpy()[keeps[k]], refs[k][keeps[k]])

    def chain(tp):
        hist = rd.TemporalHistory(tp)
        out = {}
        for k, d in enumerate(drivers):
            d.history, d._reprojected = hist, None
            img = d.denoise_temporal()
            if k in refs:
                out[k] = (err(img, k), hist.share, float(hist.length.mean()))
        return out
    last = args.frames - 1

    def score(r):
        return sum(r[k][0] for k in half) / len(half)
    say(f"Cornell with spheres {W}x{H}, {args.frames} frames of the -r animation (t = k/500) at {args.spp} spp each; error: relative L2 against {args.ref_spp} spp of the")
    say(f"same camera over the pixels whose first hit is not specular ({keeps[last].mean():.3f} of the frame)")
    say(f"`mean`: over frames {half[0]}..{last}, what a parameter set is chosen by")
    for name, img in (("noisy frames", lambda d: d.total_ob.get_pixels()), ("single-frame denoise()", lambda d: d.denoise())):
        e = {k: err(img(drivers[k]), k) for k in refs}
        say(f"  {name:24s} mean {sum(e[k] for k in half) / len(half):.4f}   frame {last}: {e[last]:.4f}   frame 2: {e[2]:.4f}")
    say()
    say(f"  {'plane_tol':>9} {'normal_cos':>10} {'alpha_min':>9} {'max_len':>7} {'floor':>6} |   mean | frame {last}: error  history  mean len | frame 2: error  history")
    start = dict(plane_tol=0.01, normal_cos=0.9, alpha_min=0.1, max_len=10.0, albedo_floor=0.02)
    results = {}

    def run(**kw):
        p = dict(start, **kw)
        key = tuple(p.values())
        if key not in results:
            r = chain(capi.TemporalParams(demodulate=1, **p))
            results[key] = r
            say(f"  {p['plane_tol']:9.4g} {p['normal_cos']:10.4g} {p['alpha_min']:9.4g} {p['max_len']:7.4g} {p['albedo_floor']:6.3g} | {score(r):.4f} |"
                f"          {r[last][0]:.4f}   {r[last][1]:.4f}   {r[last][2]:6.3f}  |          {r[2][0]:.4f}   {r[2][1]:.4f}")
        return score(results[key])
    run()
    grid = dict(plane_tol=[0.001, 0.003, 0.03, 0.1], normal_cos=[0.5, 0.8, 0.97, 0.995], alpha_min=[0.05, 0.2, 0.25, 0.34, 0.5, 0.67, 1.0],
                max_len=[2.0, 3.0, 4.0, 6.0, 32.0], albedo_floor=[0.0, 0.1, 0.25])
    best = dict(start)
    for name, values in grid.items():
        scored = [(run(), start[name])] + [(run(**{name: v}), v) for v in values]
        best[name] = min(scored)[1]
    say("  every parameter at its best single value:")
    run(**best)
    say()

    # ---- 2. kernel times at 1080p
    if not args.no_1080p:
        big = Workload("sponza-1080p", spp=1)
        g = rd.Scene(big.builder.to_desc())
        prm, tiles = big.params(), rd.generate_task_list(big.xres, big.yres)
        cam0 = big.cfg.get_camera(0.0)
        cam1 = big.cfg.get_camera(1.0 / 500.0)
        X, Y = big.xres, big.yres
        dev = torch.device("cuda", 0)

        def aov(cam):
            a = [torch.empty((Y, X, 3), dtype=torch.float32, device=dev), torch.empty((Y, X, 3), dtype=torch.float32, device=dev),
                 torch.empty((Y, X), dtype=torch.float32, device=dev), torch.empty((Y, X), dtype=torch.int32, device=dev)]
            torch.cuda.synchronize()
            g.render_aov_device(cam, prm, tiles, *[t.data_ptr() for t in a])
            return a
        a0, a1 = aov(cam0), aov(cam1)
        acc = torch.rand((Y, X, 3), dtype=torch.float32, device=dev) * 4
        cnt = torch.full((Y, X), 4, dtype=torch.int32, device=dev)
        h_rgb, h_len = torch.rand((Y, X, 3), dtype=torch.float32, device=dev), torch.full((Y, X), 5.0, dtype=torch.float32, device=dev)
        o_rgb, o_len = torch.empty_like(h_rgb), torch.empty_like(h_len)
        n_rgb, n_len, img = torch.empty_like(h_rgb), torch.empty_like(h_len), torch.empty_like(h_rgb)
        tp = capi.TemporalParams()
        g.set_tuning(time_post=1)
        torch.cuda.synchronize()
        times = []
        for r in range(3 + args.reps):
            g.temporal_reproject_device(X, Y, cam1, cam0, a1[2].data_ptr(), a1[1].data_ptr(), a1[3].data_ptr(), a0[2].data_ptr(), a0[1].data_ptr(), a0[3].data_ptr(),
                                        h_rgb.data_ptr(), h_len.data_ptr(), tp, o_rgb.data_ptr(), o_len.data_ptr())
            g.temporal_blend_device(X, Y, acc.data_ptr(), cnt.data_ptr(), a1[0].data_ptr(), o_rgb.data_ptr(), o_len.data_ptr(), tp, n_rgb.data_ptr(), n_len.data_ptr(),
                                    img.data_ptr())
            if r >= 3:
                times.append(g.post_timing(5))
        P = X * Y
        share = float((o_len > 0).double().mean())
        say(f"sponza-1080p {X}x{Y} ({big.geometry} geometry), cameras t = 0 and 1/500, history length 5 everywhere; {share:.3f} of the pixels find history;")
        say(f"{args.reps} repetitions after 3 warm-up calls, HIP events on the scene's stream, ms: median [min .. max]; byte floor at 8 TB/s")
        for k, (name, nbytes) in enumerate((("reproject", P * (20 + 4 * 36 + 16)), ("blend", P * (12 + 4 + 12 + 12 + 4 + 12 + 4 + 12)))):
            xs = [t[k] for t in times]
            floor = nbytes / 8e12 * 1e3
            say(f"  {name:10s} {statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]   byte floor {floor:.4f} ms ({nbytes / 1e6:.1f} MB): x{statistics.median(xs) / floor:.2f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
