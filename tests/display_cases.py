"""The inputs of test_gpu_display.py, made once in numpy and shared: images that reach every branch of the display stage, the calls
of rgk_display_measure_device / rgk_display_encode_device on device copies of them, and, run as a program, all of it in a process of
its own for the RGK_POISON run (python tests/display_cases.py --out FILE.npz).

    IMAGES     name -> Image: the sum plane (y, x, 3) float32 and the count plane (y, x) uint32 of one frame
    VARIANTS   name -> [(counted, mode)]: with / without the count plane (without: the sum plane itself is the image, a mean already),
               automatic exposure / a fixed exposure and white
    THRESHOLDS per operator, pixels whose channel values land on the sRGB byte thresholds and on the float below, encoded with
               hand-filled stats

The kernels stride over the frame with a bounded grid of 256-lane workgroups -- at most 1024 for the encode, 256 for the histogram
(rgk_plan.h) -- and a lane takes four pixels when the planes are 16-byte aligned (torch's allocations are) and one when they are
not.  So one pass of the encode is 1,048,576 pixels on the aligned route and 262,144 on the other, and a quarter of that for the
histogram: 1183 x 889 (1,051,687 pixels, three of them behind the last group of four) needs a second pass on the first, and
640 x 480 on planes shifted by one element needs one on the second.  The issue's 640 x 480 on aligned planes is one pass of the
encode's groups and two of the histogram's."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from rgk_amd import capi  # noqa: E402

import display_ref as D  # noqa: E402

F = np.float32
OPS = ("linear", "reinhard", "filmic")
FIXED = dict(exposure=0.5, white=2.0)           # the fixed mode's scale and white point
HAND = dict(exposure=0.7391, white=3.3)         # the threshold cases' hand-filled stats: no power of two, so the products round
PREFILL = 0x7B7B7B7B                            # what an output plane holds before a call: no word the encode writes (alpha 255)
NEW_BUFFER_BYTES = 4 * 257 + 4 * 256            # the histogram (256 bins + the dark count) and the table


class Image:
    def __init__(self, rgb, cnt, shift=0):
        self.rgb, self.cnt = np.ascontiguousarray(rgb, F), np.ascontiguousarray(cnt, np.uint32)
        self.H, self.W = self.cnt.shape
        self.shift = shift  # elements the device planes are shifted off their allocation's start: 1 -> no plane is 16-byte aligned


def edge_pixels():
    """Colours whose luminance is EXACTLY a bin edge, the float below it and the float above it, for each of the 257 edges: searched
    among seven channel patterns and the 13 floats around edge / (the pattern's coefficient sum).  (771, 3) float32; the search finds
    all of them (asserted)."""
    pats = np.array([[1, 1, 1], [1, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], F)
    coef = np.array([0.2126, 0.7152, 0.0722])
    out = []
    for b in range(257):
        e = D.edge(b)
        cand = []
        for pat in pats:
            x0 = np.array(e / (coef * pat).sum(), F)
            xs = (x0.view(np.uint32).astype(np.int64) + np.arange(-6, 7)).astype(np.uint32).view(F)
            cand.append(xs[:, None] * pat[None, :])
        cand = np.concatenate(cand).astype(F)
        Y = D.lum(cand)
        for k in (-1, 0, 1):
            hit = np.nonzero(Y == D._next(e, k))[0]
            assert len(hit), (b, k)
            out.append(cand[hit[0]])
    return np.array(out, F)


def zoo(w, h, seed):
    """Luminances log-uniform over 2^-26 .. 2^16 (below the first bin and above the last), coloured; counts 0 .. 16 with zeros; and,
    where the frame has room, NaN, -1, +inf, 1e-30 and the bin-edge pixels.  The sum plane is colour * count (exact for the special
    pixels, whose counts are 1, 2 or 4)."""
    rng = np.random.default_rng(seed)
    P = w * h
    c = (np.exp2(rng.uniform(-26, 16, (P, 1))) * rng.uniform(0.2, 1.0, (P, 3))).astype(F)
    cnt = rng.choice(np.array([0, 1, 2, 3, 4, 7, 16], np.uint32), P)
    special = np.array([[np.nan, 0.5, 0.25], [0.5, -1.0, 0.25], [np.inf, 0.1, 0.1], [1e-30, 1e-30, 1e-30], [-np.inf, np.nan, -0.0], [np.inf, np.inf, np.inf],
                        [0.0, 0.0, 0.0], [65504.0, 1e38, 3e38], [1e-45, 0.0, 1e-40]], F)
    special = np.concatenate([special, edge_pixels()])
    n = min(len(special), max(0, P - 16))  # (a 1 x 1 frame keeps its random pixel)
    if n:
        at = rng.choice(P, n, replace=False)
        c[at] = special[:n]
        cnt[at] = rng.choice(np.array([1, 2, 4], np.uint32), n)
    with np.errstate(all="ignore"):
        rgb = (c * cnt[:, None].astype(F)).astype(F)
    return Image(rgb.reshape(h, w, 3), cnt.reshape(h, w))


def constant(w, h):
    """Every pixel the same colour: one bin holds them all."""
    return Image(np.broadcast_to(np.array([0.9, 0.6, 0.3], F), (h, w, 3)), np.full((h, w), 3, np.uint32))


def black(w, h):
    """Nothing lit: every pixel is dark -- zero sums under counts that are mostly not zero."""
    cnt = np.full((h, w), 4, np.uint32)
    cnt[::3, ::5] = 0
    return Image(np.zeros((h, w, 3), F), cnt)


def make_images():
    img = {"zoo 1x1": zoo(1, 1, 1), "zoo 67x45": zoo(67, 45, 2), "zoo 96x96": zoo(96, 96, 3), "zoo 640x480": zoo(640, 480, 4),
           "zoo 1183x889": zoo(1183, 889, 5), "constant 67x45": constant(67, 45), "black 67x45": black(67, 45)}
    z = img["zoo 640x480"]
    img["zoo 640x480 unaligned"] = Image(z.rgb, z.cnt, shift=1)
    return img


ALL = [(True, "auto"), (True, "fixed"), (False, "auto"), (False, "fixed")]
VARIANTS = {"zoo 1x1": ALL, "zoo 67x45": ALL, "zoo 96x96": ALL, "zoo 640x480": ALL, "zoo 640x480 unaligned": [(True, "auto"), (False, "fixed")],
            "zoo 1183x889": [(True, "auto"), (False, "fixed")], "constant 67x45": ALL, "black 67x45": ALL}


def params_of(op, mode):
    return capi.DisplayParams(op=capi.DISPLAY_OPS[op], **(FIXED if mode == "fixed" else {}))


def threshold_image(op, T):
    """(30, 34, 3): per byte k the pair (below, at) as a grey pixel, then as the red of a pixel whose green and blue are fixed."""
    px = np.zeros((4, 255, 3), F)
    grey = D.threshold_inputs(D.OPS[op], HAND["exposure"], HAND["white"], T)
    red = D.threshold_inputs(D.OPS[op], HAND["exposure"], HAND["white"], T, others=(0.25, 0.125))
    px[0], px[1] = grey[:, :1], grey[:, 1:]
    px[2, :, 0], px[3, :, 0] = red[:, 0], red[:, 1]
    px[2:, :, 1], px[2:, :, 2] = 0.25, 0.125
    return px.reshape(30, 34, 3)


# ----------------------------------------------------------------------- the GPU side
def shifted(a, shift, dtype):
    """A device copy of `a` that starts `shift` elements into its allocation."""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1).view(dtype)
    t = torch.empty(flat.size + shift, dtype=torch.from_numpy(flat[:1]).dtype, device="cuda:0")
    t[shift:].copy_(torch.from_numpy(flat))
    return t, t[shift:]


def stats_arrays(st):
    return {"hist": np.frombuffer(st.hist, np.uint32).copy(), "counts": np.array([st.n_lit, st.n_dark], np.uint32),
            "floats": np.array([st.y_median, st.y_white, st.exposure, st.white], F)}


def gpu_encode(g, W, H, d_rgb, d_cnt, params, stats, shift=0):
    import torch
    keep, out = shifted(np.full(W * H, PREFILL, np.uint32), shift, np.int32)
    torch.cuda.synchronize()
    g.display_encode_device(W, H, d_rgb, d_cnt, params, stats, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(H, W)


def run_image(g, img, variants):
    """-> {"counted|mode::key": array}: the measured stats, and the words of the three operators encoded with them."""
    import torch
    keep_rgb, rgb = shifted(img.rgb, img.shift, F)
    keep_cnt, cnt = shifted(img.cnt, img.shift, np.int32)
    torch.cuda.synchronize()
    out = {}
    for counted, mode in variants:
        d_cnt = cnt.data_ptr() if counted else None
        for op in OPS:
            p = params_of(op, mode)
            st = g.display_measure_device(img.W, img.H, rgb.data_ptr(), d_cnt, p)
            if op == OPS[0]:
                for k, v in stats_arrays(st).items():
                    out[f"{int(counted)}|{mode}::{k}"] = v
            else:  # the measurement does not depend on the operator
                assert all(np.array_equal(v.view(np.uint32), out[f"{int(counted)}|{mode}::{k}"].view(np.uint32)) for k, v in stats_arrays(st).items())
            out[f"{int(counted)}|{mode}::{op}"] = gpu_encode(g, img.W, img.H, rgb.data_ptr(), d_cnt, p, st, img.shift)
    return out


def run_thresholds(g, T):
    import torch
    out = {}
    st = capi.DisplayStats()
    st.exposure, st.white = HAND["exposure"], HAND["white"]
    for op in OPS:
        px = threshold_image(op, T)
        H, W = px.shape[:2]
        with np.errstate(all="ignore"):
            planes = {"mean": (px, None), "counted": ((px * F(4)).astype(F), np.full((H, W), 4, np.uint32))}
        for name, (rgb, cnt) in planes.items():
            _, d_rgb = shifted(rgb, 0, F)
            d_cnt = None if cnt is None else shifted(cnt, 0, np.int32)[1]
            torch.cuda.synchronize()
            out[f"{op}|{name}"] = gpu_encode(g, W, H, d_rgb.data_ptr(), None if d_cnt is None else d_cnt.data_ptr(), capi.DisplayParams(op=capi.DISPLAY_OPS[op]), st)
    return out


def gpu_scene(rd):
    """The small Cornell fixture: it only lends its handle."""
    from rgk_amd.workloads import Workload
    return rd.Scene(Workload("cornell-256", scale=0.25, spp=4).builder)


def run_bit_cases(rd):
    """-> (images, {image: results}, {op|plane: words}, the scene, [poisoned bytes before the first display call, behind the last])."""
    import memstate_ref as M
    images = make_images()
    g = gpu_scene(rd)
    T = rd.display_table()
    before = M.poisoned()
    results = {name: run_image(g, img, VARIANTS[name]) for name, img in images.items()}
    thresholds = run_thresholds(g, T)
    return images, results, thresholds, g, [before, M.poisoned()]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from rgk_amd import render_driver as rd
    images, results, thresholds, _, poisoned = run_bit_cases(rd)
    flat = {"_poisoned": np.array(poisoned, np.uint64)}
    for name, res in results.items():
        for key, a in res.items():
            flat[f"{name}##{key}"] = a
    for key, a in thresholds.items():
        flat[f"thresholds##{key}"] = a
    np.savez(args.out, **flat)
    print("display cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
