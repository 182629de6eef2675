"""Does the a-trous filter gain from feature planes that follow mirrors and glass?  Relative L2 against a 256-spp image of a
4-spp image filtered (rgk_denoise_device, shipped defaults) once with the first-hit planes and once with the followed planes
(max_hops = 4), on the hall (tests/chain_ref.py) and on the committed Cornell box with spheres.

    python tools/aov_chain_quality.py [--cpu] [--gpu] [--out FILE]

--cpu: the oracle's images, the composed planes (tests/chain_ref.py) and the filter's numpy restatement (tests/post_ref.py).
--gpu: the library's rounds, rgk_render_aov_chain and rgk_denoise_device.  Default: --cpu, and --gpu where a device is present.
Regions: the pixels with hops > 0; of those, the ones whose chain ends on the hall's textured floor; the whole frame.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chain_ref as CR  # noqa: E402
import post_ref as R  # noqa: E402
from rgk_amd import capi  # noqa: E402

LO, HI, HOPS = 4, 256, 4


def rel(a, b, m):
    return float(np.linalg.norm(a[m].astype(np.float64) - b[m]) / np.linalg.norm(b[m].astype(np.float64)))


def case(name):
    if name == "hall":
        sb = CR.hall()
        return sb, CR.hall_camera(), CR.HALL_W, CR.HALL_H, lambda spp: CR.hall_params(spp)
    sb, cam, W, H, _, wl = CR.spheres_case()

    def prm(spp):
        p = wl.params()
        p.multisample = spp
        return p
    return sb, cam, W, H, prm


def regions(name, sb, tri, hops):
    reg = {"hops > 0": hops > 0, "whole frame": np.ones(hops.shape, bool)}
    if name == "hall":
        reg = {"hops > 0, chain ends on the floor": (hops > 0) & np.isin(tri, list(sb.parts["floor"])), **reg}
    return reg


def report(tag, name, sb, noisy, ref, first, follow, denoise):
    d = capi.DenoiseParams(sigma_color=R.default_sigma_color(*noisy, 6.0))
    img = R.mean_color(*noisy)
    den0, den1 = denoise(noisy, first, d), denoise(noisy, follow, d)
    lines = [f"{tag} {name}: {LO} spp against {HI} spp, max_hops {HOPS}, sigma_color {d.sigma_color:.4g}; relative L2: unfiltered / first-hit planes / followed planes"]
    for rn, m in regions(name, sb, follow[3], follow[4]).items():
        lines.append(f"  {rn:36s} {int(m.sum()):5d} px   {rel(img, ref, m):.4f}   {rel(den0, ref, m):.4f}   {rel(den1, ref, m):.4f}")
    return lines


def cpu(name):
    from oracle import rgk_oracle as O
    sb, cam, W, H, prm = case(name)
    desc = sb.to_desc()
    osc = O.OracleScene(desc)
    tiles = O.generate_task_list(W, H)
    noisy = osc.render_round(cam, prm(LO), tiles)[:2]
    ref = R.mean_color(*osc.render_round(cam, prm(HI), tiles)[:2])
    ch = CR.chain(O, osc, desc, cam, W, H, prm(1).bumpmap_scale, hops=HOPS)
    dn = lambda n, f, d: R.atrous_ref(n[0], n[1], f[0], f[1], f[2], d.iterations, d.sigma_color, d.sigma_depth, d.normal_power_log2, d.demodulate)
    return report("CPU (oracle, composed planes, numpy filter)", name, sb, noisy, ref, CR.planes(ch, 0), CR.planes(ch, HOPS), dn)


def gpu(name):
    import torch
    from rgk_amd import render_driver as rd
    sb, cam, W, H, prm = case(name)
    g = rd.Scene(sb.to_desc())
    tiles = rd.generate_task_list(W, H)
    noisy = g.render_round(cam, prm(LO), tiles)[:2]
    ref = R.mean_color(*g.render_round(cam, prm(HI), tiles)[:2])

    def dn(n, f, d):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        t = [up(n[0]), up(n[1].view(np.int32)), up(f[0]), up(f[1]), up(f[2])]
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        g.denoise_device(W, H, *[x.data_ptr() for x in t], d, out.data_ptr())
        return out.cpu().numpy()
    return report("GPU (rounds, rgk_render_aov_chain, rgk_denoise_device)", name, sb, noisy, ref, g.render_aov_chain(cam, prm(1), tiles, 0),
                  g.render_aov_chain(cam, prm(1), tiles, HOPS), dn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.cpu and not args.gpu:
        args.cpu = True
        args.gpu = capi.load_product().rgk_device_count() >= 1
    lines = []
    for name in ("hall", "cornell-box-spheres"):
        if args.cpu:
            lines += cpu(name)
        if args.gpu:
            lines += gpu(name)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
