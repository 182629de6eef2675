"""CPU sweep behind RenderDriver's default sigma_color (render_driver.DENOISE_SIGMA_K): the numpy restatement of the a-trous
filter (tests/post_ref.py) on the oracle's own images of the two test scenes, features composed from the oracle library.

    python tools/denoise_sweep.py [k ...]

Prints, per k, the relative L2 error of the denoised low-sample image against the high-sample one for each scene and the sum
(the table in DESIGN.md).  No GPU needed.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import post_ref as R  # noqa: E402
from oracle import rgk_oracle as O  # noqa: E402
from rgk_amd.workloads import Workload  # noqa: E402

CASES = [("cornell 96x96, 4 vs 256 spp", "cornell-256", 0.375, 4, 256), ("sponza proxy 115x64, 4 vs 128 spp", "sponza-1080p", 0.06, 4, 128)]


def case_images(name, scale, lo, hi):
    """(accumulator, counts) at `lo` samples, the image at `hi` samples, and the feature planes."""
    out = []
    for spp in (lo, hi):
        wl = Workload(name, scale=scale, spp=spp)
        desc = wl.builder.to_desc()
        osc = O.OracleScene(desc)
        acc, cnt, _ = osc.render_round(wl.camera, wl.params(), O.generate_task_list(wl.xres, wl.yres))
        out.append((acc, cnt))
        if spp == lo:
            feats = R.oracle_features(O, osc, desc, wl.camera, wl.xres, wl.yres, wl.bumpscale)
    return out[0], R.mean_color(*out[1]), feats


def main():
    ks = [float(a) for a in sys.argv[1:]] or [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0]
    data = [(label,) + case_images(name, scale, lo, hi) for label, name, scale, lo, hi in CASES]
    for label, (acc, cnt), ref, _ in data:
        level = R.default_sigma_color(acc, cnt, 1.0)
        print(f"{label}: noisy relL2 {R.rel_l2(R.mean_color(acc, cnt), ref):.4f}, mean of the largest channel {level:.4g}")
    print("k      " + "  ".join(f"{d[0].split(',')[0]:>14s}" for d in data) + "             sum   (demodulate 1 | 0)")
    for k in ks:
        row = []
        for demod in (1, 0):
            errs = []
            for _, (acc, cnt), ref, (alb, nrm, z, _) in data:
                den = R.atrous_ref(acc, cnt, alb, nrm, z, sigma_color=R.default_sigma_color(acc, cnt, k), demodulate=demod)
                errs.append(R.rel_l2(den, ref))
            row.append("  ".join(f"{e:14.4f}" for e in errs) + f"  {sum(errs):14.4f}")
        print(f"{k:<6g} " + "  |  ".join(row))


if __name__ == "__main__":
    main()
