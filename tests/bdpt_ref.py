"""The per-pixel check of a bidirectional round (reverse > 0) against the oracle's round split into its terms.  Plain numpy.

What a round adds to a pixel of a fresh accumulator (OracleScene.render_round_split keeps the parts apart):

  * `main`, the own-pixel part: the camera paths of the pixel's samples with their next-event estimates, connections and
    emission, clamped per vertex and per path and summed in sample order (PixelRenderResult::main_pixel).  One float32 value
    per channel; on the GPU it is formed by the same float operations in the same order (k_trace_shadow_jobs, k_resolve: a
    pixel's partial sample sums are carried in a side buffer, so it enters the accumulator in one piece) -- deterministic;
  * `splat_n` splats, the light-tracing side effects that project onto the pixel from ANY path of the round
    (PixelRenderResult::side_effects).  Each is one float32 value per channel; the GPU adds them with float atomics, so
    their ORDER among themselves and against `main` is free.  Splats add no sample count.

So the accumulator holds a float32 sum of 1 + splat_n known terms in an unknown order, and every pixel falls in one of three
classes:

  0. splat_n == 0: one term.  gpu == main, bit for bit.
  1. splat_n == 1 (and extra_terms == 0): two terms.  Float addition is commutative and 0 + x is exact, so there is ONE
     possible result: gpu == float32(main + splat), bit for bit.
  2. everything else, per channel:  |gpu - (float64(main) + splat_sum)| <= gamma(n) * (|main| + splat_abs),
     gamma(n) = n u / (1 - n u), u = 2^-24 (float32 unit roundoff, round to nearest), n = splat_n + extra_terms.

Derivation of (2).  Summing m = splat_n + 1 terms x_1 .. x_m into an accumulator that starts at zero takes m - 1 = splat_n
rounded additions (the first is exact).  Each rounded addition is fl(a + b) = (a + b)(1 + d), |d| <= u.  Whatever the order --
a chain, or any tree -- a term passes through at most m - 1 of them, so the computed sum is sum_i x_i (1 + t_i) with
|1 + t_i| <= (1 + u)^(m-1), i.e. |t_i| <= gamma(m - 1) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Lemma 3.1 and (4.4)), and the error is at most gamma(m - 1) * sum_i |x_i|.  With m - 1 = splat_n that is the bound above:
derived, not measured, and it gets no slack.  The reference value float64(main) + splat_sum is exact to 2^-53 relative per
addition, nine orders of magnitude below u.

extra_terms.  A plan that splits a pixel's samples over several passes could hand the own-pixel part to the accumulator in up to
`multisample` pieces; callers pass extra_terms = multisample for such plans, one more rounded addition per piece in n.  Class 1
then no longer has a single possible result and is held to the bound; class 0 stays exact (the product carries a pixel's partial
sample sums in a side buffer and adds the own-pixel part once, in sample order).  A second round onto the first round's
accumulator needs no extra_terms: hand the second round's own-pixel part over as one more order-free term of every pixel
(add_term) -- two rounds without splats are then class 1, float32(main_1 + main_2) exactly.

Sample counts are exactly the oracle's, and where the oracle's terms are finite and non-negative the GPU's sum is too."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _bits(a):
    """float32 bit patterns with -0 folded onto +0 (0 + -0 = +0 in an accumulator, -0 alone in a plane of terms)."""
    return (np.asarray(a, np.float32) + np.float32(0.0)).view(np.uint32)


def check_round(gpu_rgb, gpu_count, main, splat_sum, splat_abs, splat_n, count_ref, extra_terms=0):
    """Per-pixel verdict planes and a summary (module docstring).  Planes: `cls` (0, 1, 2), `ok` (bool), `ratio`
    (error / bound, the worst channel; 0 or inf in the bit-exact classes and where the bound is 0), `bad_value` (NaN or negative
    where the oracle has none).  Summary: share_n0 / share_n1 / share_bound, exact_n0 / exact_n1 (share of the class that is
    bit-exact; 1.0 for an empty class), worst_ratio (over class 2), outside (pixels not ok), counts_equal, bad_values, pixels."""
    gpu = np.asarray(gpu_rgb, np.float32)
    main = np.asarray(main, np.float32)
    splat_sum, splat_abs = np.asarray(splat_sum, np.float64), np.asarray(splat_abs, np.float64)
    splat_n = np.asarray(splat_n)
    assert gpu.shape == main.shape == splat_sum.shape == splat_abs.shape and gpu.shape[:2] == splat_n.shape
    n = splat_n.astype(np.float64) + float(extra_terms)
    cls = np.full(splat_n.shape, 2, np.uint8)
    cls[splat_n == 0] = 0
    if extra_terms == 0:
        cls[splat_n == 1] = 1
    # classes 0 and 1: the one possible float32 result
    one = np.where((splat_n == 0)[..., None], main, main + splat_sum.astype(np.float32))   # (one splat: splat_sum IS that float32 value)
    same = (_bits(gpu) == _bits(one)).all(axis=2)
    # class 2: the summation-order bound
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(gpu.astype(np.float64) - (main.astype(np.float64) + splat_sum))
        bound = gamma(n)[..., None] * (np.abs(main.astype(np.float64)) + splat_abs)
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=2)
    ref_clean = (np.isfinite(main) & (main >= 0) & np.isfinite(splat_sum) & (splat_sum >= 0)).all(axis=2)
    bad_value = ref_clean & ~(np.isfinite(gpu) & (gpu >= 0)).all(axis=2)
    ok = np.where(cls == 2, ratio <= 1.0, same) & ~bad_value
    ratio = np.where(cls == 2, ratio, np.where(same, 0.0, np.inf))
    counts_equal = bool(np.array_equal(np.asarray(gpu_count), np.asarray(count_ref)))

    def share(m, of=None):
        d = ok.size if of is None else int(of.sum())
        return float(m.sum() / d) if d else 1.0
    c0, c1, c2 = cls == 0, cls == 1, cls == 2
    summary = dict(share_n0=share(c0), share_n1=share(c1), share_bound=share(c2), exact_n0=share(c0 & same, c0), exact_n1=share(c1 & same, c1),
                   worst_ratio=float(ratio[c2].max()) if c2.any() else 0.0, outside=int((~ok).sum()), outside_n0=int((~ok & c0).sum()),
                   outside_n1=int((~ok & c1).sum()), outside_bound=int((~ok & c2).sum()), counts_equal=counts_equal,
                   bad_values=int(bad_value.sum()), pixels=int(ok.size))
    return dict(cls=cls, ok=ok, ratio=ratio, bad_value=bad_value), summary


def check_split(gpu_rgb, gpu_count, split, extra_terms=0):
    """check_round on what OracleScene.render_round_split returned."""
    return check_round(gpu_rgb, gpu_count, split.main, split.splat_sum, split.splat_abs, split.splat_n, split.count, extra_terms)


def add_term(split, term):
    """The planes of `split` with one more float32 term per pixel among the order-free ones (a second round's own-pixel part):
    (main, splat_sum, splat_abs, splat_n)."""
    t = np.asarray(term, np.float32).astype(np.float64)
    return split.main, split.splat_sum + t, split.splat_abs + np.abs(t), split.splat_n + np.uint32(1)


def record_fields(summary):
    """What the GPU tests hand to record_parity: class shares, the worst error / bound, the pixels outside."""
    return dict(n0=summary["share_n0"], n1=summary["share_n1"], bound=summary["share_bound"], worst_err_over_bound=summary["worst_ratio"],
                outside=summary["outside"], pixels=summary["pixels"])


def planes_from_list(splats, shape):
    """(splat_sum, splat_abs, splat_n) of a splat list (records x, y, rgb) -- what render_round_split forms itself."""
    s, a, n = np.zeros(shape + (3,), np.float64), np.zeros(shape + (3,), np.float64), np.zeros(shape, np.uint32)
    rgb = splats["rgb"].astype(np.float64)
    np.add.at(s, (splats["y"], splats["x"]), rgb)
    np.add.at(a, (splats["y"], splats["x"]), np.abs(rgb))
    np.add.at(n, (splats["y"], splats["x"]), 1)
    return s, a, n


def resum_in_round_order(split, tiles):
    """main + splats added in float32 in orc_render_round's own order: per task its own pixels, then its splats in list order."""
    acc = np.zeros_like(split.main)
    for i, t in enumerate(tiles):
        acc[t.y0:t.y1, t.x0:t.x1] += split.main[t.y0:t.y1, t.x0:t.x1]
        s = split.splats[split.splats["task"] == i]
        np.add.at(acc, (s["y"], s["x"]), s["rgb"])          # unbuffered: one at a time, in list order
    return acc


def resum_in_random_order(split, rng):
    """Every pixel's terms (main where the pixel was rendered, and its splats) added in float32 in a random order."""
    ys, xs = np.nonzero(split.count > 0)
    ty = np.concatenate([ys, split.splats["y"]]); tx = np.concatenate([xs, split.splats["x"]])
    tv = np.concatenate([split.main[ys, xs], split.splats["rgb"]]).astype(np.float32)
    acc = np.zeros_like(split.main)
    k = rng.permutation(len(ty))
    np.add.at(acc, (ty[k], tx[k]), tv[k])
    return acc
