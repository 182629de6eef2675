"""CPU sweep behind the shipped sigma_k and albedo_floor of the variance-guided filter (capi.DenoiseVarParams), and the calibration
of the half-buffer noise estimate: the numpy restatement (tests/noise_ref.py) on the oracle's own images of the two test scenes,
two halves of 2 spp with tile seeds from seedstart 42 and 100042, features composed from the oracle library.

    python tools/noise_sweep.py

Prints the noisy and fixed-sigma errors, the table sigma_k x albedo_floor of relative L2 errors against the high-sample image per
scene and summed, and per scene the calibration of the raw variance plane: sum(v) / sum|c - ref|^2 and the estimated
relative noise over the measured relative L2 error.  No GPU needed.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import noise_ref as N  # noqa: E402
import post_ref as R  # noqa: E402
from oracle import rgk_oracle as O  # noqa: E402

SIGMA_K = [1.0, 2.0, 3.0, 4.0, 6.0]
FLOORS = [1.0 / 256, 1.0 / 64, 1.0 / 16, 1.0 / 4]


def main():
    data = [(label,) + N.oracle_case(O, name, scale, lo, hi) for label, name, scale, lo, hi in N.CASES]
    for label, (S, n, SB, nB), ref, (alb, nrm, z, _) in data:
        c = R.mean_color(S, n)
        fixed = R.atrous_ref(S, n, alb, nrm, z, sigma_color=R.default_sigma_color(S, n, 6.0))
        print(f"{label}: noisy relL2 {R.rel_l2(c, ref):.4f}, fixed-sigma filter (k = 6, demodulate 1) {R.rel_l2(fixed, ref):.4f}")
        v = N.raw_variance(S, n, SB, nB).astype(np.float64)
        err2 = ((c.astype(np.float64) - ref) ** 2).sum()
        sums, _ = N.noise_tiles(S, n, SB, nB, 32)
        print(f"    calibration: sum(v) / sum|c - ref|^2 = {v.sum() / err2:.4f}; estimated relative noise {N.rel_noise(sums):.4f} / measured {R.rel_l2(c, ref):.4f}"
              f" = {N.rel_noise(sums) / R.rel_l2(c, ref):.4f}")
    names = "  ".join(f"{d[0].split(',')[0]:>14s}" for d in data)
    for demod in (1, 0):
        print(f"\ndemodulate {demod}\nsigma_k  floor      {names}             sum")
        for k in SIGMA_K:
            for fl in (FLOORS if demod else FLOORS[:1]):
                errs = []
                for _, (S, n, SB, nB), ref, (alb, nrm, z, _) in data:
                    den, _ = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, sigma_k=k, albedo_floor=fl, demodulate=demod)
                    errs.append(R.rel_l2(den, ref))
                print(f"{k:<7g}  {('1/%d' % round(1 / fl)) if demod else '-':<9s}  " + "  ".join(f"{e:14.4f}" for e in errs) + f"  {sum(errs):14.4f}")


if __name__ == "__main__":
    main()
