"""Quality of the demodulated route (RenderDriver(track_demod=True): denoise() and upsample()) beside the shipped routes, on one GPU.

    python tools/demod_quality.py [--low-spp 64] [--ref-spp 1024] [--out FILE]

Upsampling: the three inputs of profiles/upsample_quality.txt -- Cornell with spheres 96x96 from 24x24, the Sponza proxy 192x108 from
48x27 and 384x216 from 96x54 -- the low grid at `low-spp` samples, relative L2 against `ref-spp` samples at full resolution over all
pixels, no filter: the plain bilinear upscale, the shipped upsampler (no albedo division), the shipped upsampler with its centre-ray
division switched on (floor 0.02: what DESIGN.md 17 measured at x3.4 on the proxy), and the demodulated route at each floor.
Denoising: the inputs and sample counts of DESIGN.md 11's table -- Cornell 96x96 at 4 against 256 spp, the Sponza proxy 115x64 at 4
against 128 spp -- the noisy image, the shipped filter (demodulate = 1: the mean over the centre ray's albedo) and the demodulated
route at each floor, all on the same rounds (a track_demod driver's accumulator is the plain driver's, bit for bit).
The floor sweep is 0, 0.02, 0.1, 0.25; the last lines give each floor's mean ratio to the shipped route.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOORS = (0.0, 0.02, 0.1, 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--low-spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from rgk_amd import capi, render_driver as rd
    from rgk_amd.workloads import Workload
    import upsample_cases as UC
    import upsample_ref as U

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rel_l2(a, b):
        return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))
    ratios = {f: [] for f in FLOORS}

    say(f"UPSAMPLING: low grid at {args.low_spp} spp, reference {args.ref_spp} spp at full resolution; relative L2 over all pixels; no filter")
    say(f"  {'input':36s} {'bilinear':>9s} {'shipped':>9s} {'centre-ray division':>20s} | demodulated route at floor " + "  ".join(f"{f:>7.3g}" for f in FLOORS))
    for scene, full in (("spheres", (96, 96)), ("sponza", (192, 108)), ("sponza", (384, 216))):
        low = (full[0] // 4, full[1] // 4)
        sc = UC.SceneSet(scene)
        g = rd.Scene(sc.builder.to_desc())
        ref_drv = rd.RenderDriver(g, sc.cfg(*full, args.ref_spp), sc.camera(*full))
        ref_drv.render_round()
        ref = ref_drv.total_ob.get_pixels().cpu().numpy()
        aov = ref_drv.render_aov()
        cam = sc.camera(*full)
        plain = rd.RenderDriver(g, sc.cfg(*low, args.low_spp), sc.camera(*low))
        plain.render_round()
        bil = U.bilinear_ref(cam, aov["normal"].cpu().numpy(), aov["depth"].cpu().numpy(), plain.camera, plain.total_ob.get_pixels().cpu().numpy())
        e_bil = rel_l2(bil, ref)
        e_ship = rel_l2(plain.upsample(cam, *full)[0].cpu().numpy(), ref)
        e_div = rel_l2(plain.upsample(cam, *full, capi.UpsampleParams(demodulate=1, albedo_floor=0.02))[0].cpu().numpy(), ref)
        es = []
        for f in FLOORS:
            drv = rd.RenderDriver(g, sc.cfg(*low, args.low_spp), sc.camera(*low), track_demod=True, albedo_floor=f)
            drv.render_round()
            assert np.array_equal(drv.total_ob.data.cpu().numpy(), plain.total_ob.data.cpu().numpy())
            es.append(rel_l2(drv.upsample(cam, *full)[0].cpu().numpy(), ref))
            ratios[f].append(es[-1] / e_ship)
        say(f"  {scene + f' {full[0]}x{full[1]} from {low[0]}x{low[1]}':36s} {e_bil:9.5f} {e_ship:9.5f} {e_div:20.5f} | " + " " * 27 + "  ".join(f"{e:7.5f}" for e in es))
        say(f"  {'  ratio to the shipped upsampler':36s} {e_bil / e_ship:9.4f} {1.0:9.4f} {e_div / e_ship:20.4f} | " + " " * 27 + "  ".join(f"{e / e_ship:7.4f}" for e in es))
        g.close()

    say()
    say("DENOISING: shipped defaults (5 iterations, sigma_color = 6 x the image's level); relative L2 against the high-sample image over all pixels")
    say(f"  {'input':44s} {'noisy':>9s} {'shipped':>9s} | demodulated route at floor " + "  ".join(f"{f:>7.3g}" for f in FLOORS))
    for name, scale, lo, hi in (("cornell-256", 0.375, 4, 256), ("sponza-1080p", 0.06, 4, 128)):
        wl = Workload(name, scale=scale, spp=lo)
        g = rd.Scene(wl.builder.to_desc())

        def cfg_of(spp):
            w = Workload(name, scale=scale, spp=spp)
            prm = w.params()

            class Cfg:
                xres, yres, render_rounds, render_minutes = w.xres, w.yres, 1, None
                get_params = staticmethod(lambda sampler=0, flags=0: prm)
            return Cfg
        ref_drv = rd.RenderDriver(g, cfg_of(hi), wl.camera)
        ref_drv.render_round()
        ref = ref_drv.total_ob.get_pixels().cpu().numpy()
        plain = rd.RenderDriver(g, cfg_of(lo), wl.camera)
        plain.render_round()
        e_noisy = rel_l2(plain.total_ob.get_pixels().cpu().numpy(), ref)
        e_ship = rel_l2(plain.denoise().cpu().numpy(), ref)
        es = []
        for f in FLOORS:
            drv = rd.RenderDriver(g, cfg_of(lo), wl.camera, track_demod=True, albedo_floor=f)
            drv.render_round()
            assert np.array_equal(drv.total_ob.data.cpu().numpy(), plain.total_ob.data.cpu().numpy())
            es.append(rel_l2(drv.denoise().cpu().numpy(), ref))
            ratios[f].append(es[-1] / e_ship)
        label = f"{name} {wl.xres}x{wl.yres}, {lo} vs {hi} spp ({wl.geometry} geometry)"
        say(f"  {label:44s} {e_noisy:9.5f} {e_ship:9.5f} | " + " " * 27 + "  ".join(f"{e:7.5f}" for e in es))
        say(f"  {'  ratio to the shipped filter':44s} {e_noisy / e_ship:9.4f} {1.0:9.4f} | " + " " * 27 + "  ".join(f"{e / e_ship:7.4f}" for e in es))
        g.close()

    say()
    say("mean ratio to the shipped route over the five inputs, per floor (below 1: the demodulated route is closer to the reference):")
    for f in FLOORS:
        say(f"  floor {f:5.3g}: {sum(ratios[f]) / len(ratios[f]):.4f}   (upsampling {sum(ratios[f][:3]) / 3:.4f}, denoising {sum(ratios[f][3:]) / 2:.4f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
