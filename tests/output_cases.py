"""The inputs of test_gpu_output.py, made once in numpy and shared: frames for rgk_output_write_exr_device and
rgk_output_write_png_device, the calls on device copies of them, the same files through the host writers (the reference), and, run
as a program, all the device calls in a process of its own for the RGK_POISON run (python tests/output_cases.py --out FILE.npz).

    exr_cases()  [ExrCase]: name, the sum plane (y, x, 3) float32, the count plane (y, x) uint32 or None (image mode), output_scale
    png_cases()  [(name, (y, x) uint32 words)]

Shapes are the smallest at which the kernels can still go wrong.  k_out_pack_exr gives a lane two adjacent pixels and a workgroup 512
of a line: 1 x 1 and 3 x 2 are the odd-xres route with a lane of one pixel, 64 x 1 half a wave of dword stores, 65 x 3 and 67 x 45 a
wave and a lane-pair tail on the narrow route, 130 x 5 the even route past one wave, 514 x 3 two workgroups per line; 600 x 656 holds
the whole half-boundary set once and is the one frame with more pixels than k_out_max has lanes in flight (1024 x 256), so its
second pass runs.  k_out_pack_png and k_out_png_sums: one to three stored blocks, the last dword of the payload cut at every
length modulo 4 among the sizes, raw byte 65535 a filter byte, an R, a G and a B, and up to 33 pieces per checksum."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctypes as C  # noqa: E402

from rgk_amd import capi  # noqa: E402

import memstate_ref as M  # noqa: E402

F = np.float32
W, H = M.W, M.H
SCALE = 0.0573
COUNTS = np.array([0, 1, 3, 256, (1 << 24) + 1], np.uint32)
SHAPES = [(1, 1), (3, 2), (64, 1), (65, 3), (130, 5), (514, 3)]
SEGMENT = 4096          # RGK_PACK_SEGMENT
MAX_WGS = 1024          # RGK_OUT_MAX_WGS


# ----------------------------------------------------------------------- the half-boundary set
def half_boundary_values():
    """float32: every half value, the float midpoints between neighbouring halves, 2^-25, 65520 and 65536 -- each with its two
    float neighbours and in both signs -- then zeros, infinities, and quiet and signalling NaNs with low and high payload bits."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(F)
    up = np.append(h[1:], F(65536.0))
    mid = (h.astype(np.float64) + up.astype(np.float64)) / 2  # exact in float32: twelve significant bits
    assert (mid.astype(F).astype(np.float64) == mid).all()
    base = np.concatenate([h, mid.astype(F), np.array([0x33000000, 0x33000001, 0x477FEFFF, 0x477FF000], np.uint32).view(F)]).view(np.uint32)
    pos = np.concatenate([base - 1, base, base + 1]) & 0x7FFFFFFF
    nans = np.array([0x7F800000, 0x7FC00000, 0x7FC00001, 0x7FFFFFFF, 0x7FE00000, 0x7F800001, 0x7F801FFF, 0x7F802000, 0x7FBFFFFF, 0x7FA00000], np.uint32)
    pos = np.unique(np.concatenate([pos, nans]))
    return np.concatenate([pos, pos | 0x80000000]).astype(np.uint32).view(F)


class ExrCase:
    def __init__(self, name, rgb, cnt, scale):
        self.name, self.rgb, self.cnt, self.scale = name, np.ascontiguousarray(rgb, F), None if cnt is None else np.ascontiguousarray(cnt, np.uint32), float(scale)
        self.H, self.W = self.rgb.shape[:2]


def synthetic(w, h, seed, wild):
    """Sums and counts: counts of 0, 1, 3, 256 and 2^24 + 1; random values with negatives; where the count is 1, values from the
    half-boundary set; -0 and NaN; `wild` adds both infinities (which make the auto scale 0)."""
    rng = np.random.default_rng(seed)
    P = w * h
    cnt = COUNTS[rng.integers(0, len(COUNTS), P)] if P > 4 else COUNTS[(np.arange(P) + 1 + seed) % len(COUNTS)]
    rgb = (np.exp2(rng.uniform(-28, 18, (P, 3))) * rng.choice([-1.0, 1.0, 1.0, 1.0], (P, 3))).astype(F)
    B = half_boundary_values()
    one = np.flatnonzero(cnt == 1)
    rgb[one] = B[rng.integers(0, len(B), (len(one), 3))]
    special = [-0.0, np.nan, 0.0] + ([np.inf, -np.inf] if wild else [])
    at = rng.choice(P * 3, min(len(special), P * 3), replace=False)
    rgb.reshape(-1)[at] = np.array(special, F)[:len(at)]
    if not wild:
        rgb[np.isinf(rgb)] = 65504.0
    return rgb.reshape(h, w, 3), cnt.reshape(h, w)


def exr_cases(cornell=None):
    """cornell: (sums, counts) of a rendered 67 x 45 frame, host arrays; None: the synthetic cases alone."""
    cases = []
    for i, (w, h) in enumerate(SHAPES):
        tame, wild = synthetic(w, h, 10 + i, False), synthetic(w, h, 20 + i, True)
        cases += [ExrCase(f"{w}x{h} accum auto", *tame, -1.0), ExrCase(f"{w}x{h} accum auto wild", *wild, 0.0), ExrCase(f"{w}x{h} accum scale 1", *wild, 1.0),
                  ExrCase(f"{w}x{h} accum fixed", *wild, SCALE), ExrCase(f"{w}x{h} image scale 1", wild[0], None, 1.0),
                  ExrCase(f"{w}x{h} image fixed", wild[0], None, SCALE)]
    B = half_boundary_values()
    bw, bh = 600, 656
    assert bw * bh * 3 >= len(B) and bw * bh > MAX_WGS * 256
    whole = np.resize(B, bw * bh * 3).reshape(bh, bw, 3)
    cases += [ExrCase("boundary set accum count 1 scale 1", whole, np.ones((bh, bw), np.uint32), 1.0), ExrCase("boundary set image scale 1", whole, None, 1.0),
              ExrCase("boundary set accum auto", np.where(np.isfinite(whole), np.abs(whole), F(1)), np.full((bh, bw), 3, np.uint32), -1.0)]
    rng = np.random.default_rng(5)
    cases.append(ExrCase("67x45 no sample anywhere", rng.random((H, W, 3)), np.zeros((H, W), np.uint32), -1.0))
    if cornell is not None:
        acc, cnt = cornell
        with np.errstate(all="ignore"):
            mean = np.where(cnt[..., None] > 0, acc / np.maximum(cnt, 1)[..., None].astype(F), F(0)).astype(F)
        cases += [ExrCase("cornell accum auto", acc, cnt, -1.0), ExrCase("cornell accum fixed", acc, cnt, SCALE), ExrCase("cornell image scale 1", mean, None, 1.0),
                  ExrCase("cornell image fixed", mean, None, SCALE)]
    return cases


def boundary_sizes():
    """Per kind of raw byte 65535 -- filter byte, R, G, B -- the first xres from 28 on that puts it there, with rows past it."""
    found = {}
    for xres in range(28, 200):
        c = 65535 % (3 * xres + 1)
        found.setdefault("filter" if c == 0 else "RGB"[(c - 1) % 3], (xres, 65535 // (3 * xres + 1) + 3))
    assert sorted(found) == ["B", "G", "R", "filter"] and found["filter"] == (28, 774)
    return found


def png_cases():
    sizes = [("1x1", 1, 1), ("3x2", 3, 2), ("67x45", W, H), ("150x150 two blocks", 150, 150), ("211x211 three blocks", 211, 211)]
    sizes += [(f"{w}x{h} byte 65535 is {kind}", w, h) for kind, (w, h) in sorted(boundary_sizes().items())]
    rng = np.random.default_rng(6)
    return [(name, rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)) for name, w, h in sizes]


# ----------------------------------------------------------------------- what the device buffer must grow by
def exr_device_bytes(w, h):
    data = h * (8 + 8 * w)
    return ((data + 4 + 15) & ~15) + 4 * MAX_WGS


def png_device_bytes(w, h):
    raw = (3 * w + 1) * h
    payload = 2 + raw + 5 * -(-raw // 65535)
    return ((payload + 3) & ~3) + 4 * (2 * -(-raw // SEGMENT) + -(-(payload + 4) // SEGMENT))


def grown_bytes(needs):
    """What a DevBuf that only grows allocates -- and RGK_POISON fills -- over a sequence of requests."""
    have = total = 0
    for n in needs:
        if n > have:
            have, total = n, total + n
    return total


# ----------------------------------------------------------------------- the reference: the host writers
def host_exr(case, path):
    """-> (file bytes, scale used): rgk_output_normalize + rgk_output_write_exr, or (image * scale) + rgk_output_write_exr."""
    lib = capi.load_product()
    val = C.c_float(case.scale)
    if case.cnt is None:
        with np.errstate(all="ignore"):
            out = (case.rgb * F(case.scale)).astype(F)
    else:
        out = np.empty_like(case.rgb)
        capi.check(lib, lib.rgk_output_normalize(case.rgb.ctypes.data, case.cnt.ctypes.data, case.W, case.H, case.scale, out.ctypes.data, C.byref(val)))
    capi.check(lib, lib.rgk_output_write_exr(str(path).encode(), case.W, case.H, out.ctypes.data))
    return np.fromfile(str(path), np.uint8), np.array([val.value], F)


def host_png(words, path):
    lib = capi.load_product()
    capi.check(lib, lib.rgk_output_write_png(str(path).encode(), words.shape[1], words.shape[0], np.ascontiguousarray(words).ctypes.data))
    return np.fromfile(str(path), np.uint8)


# ----------------------------------------------------------------------- the GPU side
def device_exr(g, case, path):
    import torch
    rgb = M.up(case.rgb)
    cnt = None if case.cnt is None else M.up(case.cnt)
    torch.cuda.synchronize()
    val = g.write_exr_device(path, case.W, case.H, rgb.data_ptr(), None if cnt is None else cnt.data_ptr(), case.scale)
    return np.fromfile(str(path), np.uint8), np.array([val], F)


def device_png(g, words, path):
    import torch
    t = M.up(words)
    torch.cuda.synchronize()
    g.write_png_device(path, words.shape[1], words.shape[0], t.data_ptr())
    return np.fromfile(str(path), np.uint8)


def cornell_scene(rd):
    """A handle of the Cornell box with a point light, its camera at 67 x 45 and the parameters of two rounds."""
    sb, cam = M._cornell("point")()
    return rd.Scene(sb), cam, M.params()


def render_rounds(rd, g, cam, prm, rounds=2, between=None):
    """-> (sums, counts) torch tensors on the device after `rounds` rounds of one frame; between(acc, cnt) runs after the first."""
    import torch
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    tiles = rd.generate_task_list(W, H)
    for r in range(rounds):
        torch.cuda.synchronize()
        g.render_round_device(cam, prm, rd.generate_task_list(W, H, seedcount_base=r * len(tiles)), acc.data_ptr(), cnt.data_ptr())
        if r == 0 and between:
            between(acc, cnt)
    torch.cuda.synchronize()
    return acc, cnt


def run_device_cases(rd, tmp):
    """-> ({key: array}, the scene and its camera and parameters, the cases, [poisoned bytes before the first output call, behind the
    last]).  The frame is rendered first: the rounds' own allocations are not the output path's."""
    g, cam, prm = cornell_scene(rd)
    acc, cnt = render_rounds(rd, g, cam, prm)
    exrs = exr_cases((acc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)))
    pngs = png_cases()
    before = M.poisoned()
    out = {}
    for c in exrs:
        out[f"exr##{c.name}"], out[f"exr##{c.name}##scale"] = device_exr(g, c, os.path.join(str(tmp), "d.exr"))
    for name, words in pngs:
        out[f"png##{name}"] = device_png(g, words, os.path.join(str(tmp), "d.png"))
    return out, (g, cam, prm), (exrs, pngs), [before, M.poisoned()]


def expected_growth(exrs, pngs):
    return grown_bytes([exr_device_bytes(c.W, c.H) for c in exrs] + [png_device_bytes(w.shape[1], w.shape[0]) for _, w in pngs])


def main(argv=None):
    import tempfile
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from rgk_amd import render_driver as rd
    with tempfile.TemporaryDirectory() as tmp:
        out, _, _, poisoned = run_device_cases(rd, tmp)
    np.savez(args.out, _poisoned=np.array(poisoned, np.uint64), **out)
    print("output cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
