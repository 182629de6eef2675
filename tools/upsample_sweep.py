"""Quality of the guided upsampler over its parameters, on one GPU.

    python tools/upsample_sweep.py [--low-spp 64] [--ref-spp 1024] [--size NAME W H]... [--out FILE]

The two inputs of the quality test (tests/upsample_cases.py QUALITY_CASES): the low grid -- a quarter of the full size on each axis,
with the camera -p would make -- rendered at `low-spp` samples so that what is measured is reconstruction, not noise, and upsampled
to the full grid without a filter.  Error: relative L2 against `ref-spp` samples at full resolution of the same camera, over all
pixels.  Beside it the plain bilinear upscale of the same low image through the same projection (tests/upsample_ref.py
bilinear_ref) and the shares of pixels by support.  One parameter at a time around the starting values, then pairs.
--size replaces a case's full size (the low size follows), to see how the shares move with the resolution.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--low-spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--size", nargs=3, action="append", default=[], metavar=("NAME", "W", "H"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from rgk_amd import capi, render_driver as rd
    import upsample_cases as UC
    import upsample_ref as U

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rel_l2(a, b):
        return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))
    cases = []
    for name, (scene, full, low) in UC.QUALITY_CASES.items():
        sizes = [(int(w), int(h)) for n, w, h in args.size if n == scene] or [full]
        cases += [(scene, s, (s[0] // 4, s[1] // 4)) for s in sizes]
    start = dict(plane_tol=0.01, normal_cos=0.9, demodulate=1, albedo_floor=0.02)
    shipped = capi.UpsampleParams()
    shipped = dict(plane_tol=round(shipped.plane_tol, 6), normal_cos=round(shipped.normal_cos, 6), demodulate=shipped.demodulate, albedo_floor=round(shipped.albedo_floor, 6))
    sets = [shipped, start]
    sets += [dict(start, plane_tol=v) for v in (0.0025, 0.005, 0.02, 0.05, 0.1, 1.0)]
    sets += [dict(start, normal_cos=v) for v in (-1.0, 0.0, 0.5, 0.7, 0.8, 0.95, 0.99)]
    sets += [dict(start, albedo_floor=v) for v in (0.0, 0.005, 0.1, 0.25)]
    sets += [dict(start, demodulate=0)]
    sets += [dict(start, plane_tol=pt, normal_cos=nc) for pt in (0.02, 0.05) for nc in (0.0, 0.5, 0.7)]
    # the geometric tests again where the albedo division is weak or off: it dominates the error at the starting floor
    sets += [dict(plane_tol=pt, normal_cos=nc, demodulate=dm, albedo_floor=fl) for dm, fl in ((0, 0.02), (1, 0.25), (1, 0.5), (1, 1.0))
             for nc in (-1.0, 0.0, 0.5, 0.9) for pt in (0.01, 0.05, 1.0)]
    sets += [dict(plane_tol=pt, normal_cos=nc, demodulate=0, albedo_floor=0.02) for nc in (-1.0, 0.0) for pt in (0.02, 0.03, 0.075, 0.1, 0.2)]
    say(f"low grid at {args.low_spp} spp, reference {args.ref_spp} spp at full resolution; relative L2 over all pixels; no filter")
    total = {}
    for scene, full, low in cases:
        sc = UC.SceneSet(scene)
        g = rd.Scene(sc.builder.to_desc())
        low_drv = rd.RenderDriver(g, sc.cfg(*low, args.low_spp), sc.camera(*low))
        low_drv.render_round()
        ref_drv = rd.RenderDriver(g, sc.cfg(*full, args.ref_spp), sc.camera(*full))
        ref_drv.render_round()
        ref = ref_drv.total_ob.get_pixels().cpu().numpy()
        aov = ref_drv.render_aov()
        cam = sc.camera(*full)
        plain = U.bilinear_ref(cam, aov["normal"].cpu().numpy(), aov["depth"].cpu().numpy(), low_drv.camera, low_drv.total_ob.get_pixels().cpu().numpy())
        e_plain = rel_l2(plain, ref)
        say()
        say(f"{scene} {full[0]}x{full[1]} from {low[0]}x{low[1]}: bilinear upscale {e_plain:.5f}")
        say(f"  {'plane_tol':>9} {'normal_cos':>10} {'demod':>5} {'floor':>6} |  guided   ratio | support 0       1       2")
        seen = set()
        for k, p in enumerate(sets):
            key = tuple(sorted(p.items()))
            if key in seen and k > 1:
                continue
            seen.add(key)
            rgb, sup = low_drv.upsample(cam, *full, capi.UpsampleParams(**p))
            rgb, sup = rgb.cpu().numpy(), sup.cpu().numpy()
            e = rel_l2(rgb, ref)
            tag = "  <- shipped" if k == 0 else ("  <- starting values" if k == 1 else "")
            say(f"  {p['plane_tol']:9.4g} {p['normal_cos']:10.3g} {p['demodulate']:5d} {p['albedo_floor']:6.3g} | {e:.5f}  {e / e_plain:.4f} | "
                f"{(sup == 0).mean():.4f}  {(sup == 1).mean():.4f}  {(sup == 2).mean():.4f}{tag}")
            total.setdefault(key, []).append(e / e_plain)
        g.close()
    say()
    say("mean ratio over the inputs, best first:")
    for key, rs in sorted(total.items(), key=lambda kv: sum(kv[1]) / len(kv[1]))[:8]:
        say(f"  {dict(key)}: {sum(rs) / len(rs):.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
