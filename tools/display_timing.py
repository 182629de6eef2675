"""What the display stage costs, on one GPU, and that the plain round did not move.

    python tools/display_timing.py [--workload sponza-1080p] [--reps 20] [--warmup 3] [--parent-tree DIR] [--out FILE]

The display leg (a process of its own): the workload's frame, one round at 8 spp for an accumulator with a real image in it, then per
operator `reps` calls of rgk_display_measure_device + rgk_display_encode_device after `warmup`, timed by HIP events on the scene's
stream ("time_post": rgk_scene_get_post_timing 10 and 11), median [min .. max]; beside them their byte floors at 8 TB/s (16 B per
pixel read by the measure; 16 B read and 4 B written by the encode) and the a-trous denoise call of the same process on the same
frame (rgk_scene_get_post_timing 1, its launches summed).
The plain round, with --parent-tree (a checkout of the parent commit with its library built): tools/demod_timing.py's plain leg on
this tree and on that one, alternating this / parent / this / parent in one session, each leg a process of its own; the parent's
own spread over its two legs says what run-to-run variation is.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("linear", "reinhard", "filmic")


def leg(args):
    """The display child; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import torch
    from rgk_amd import capi
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import Workload
    wl = Workload(args.workload, scale=args.scale, spp=8)
    scene = rd.Scene(wl.builder.to_desc())
    prm = wl.params()
    W, H = wl.xres, wl.yres
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    out = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    tiles = rd.generate_task_list(W, H)
    torch.cuda.synchronize()
    scene.render_round_device(wl.camera, prm, tiles, acc.data_ptr(), cnt.data_ptr())
    scene.set_tuning(time_post=1)
    res = dict(size=[W, H], geometry=wl.geometry, clear=[], hist=[], encode={op: [] for op in OPS})
    for op in OPS:
        p = capi.DisplayParams(op=capi.DISPLAY_OPS[op])
        for r in range(args.warmup + args.reps):
            st = scene.display_measure_device(W, H, acc.data_ptr(), cnt.data_ptr(), p)
            t10 = scene.post_timing(10)
            scene.display_encode_device(W, H, acc.data_ptr(), cnt.data_ptr(), p, st, out.data_ptr())
            t11 = scene.post_timing(11)
            if r >= args.warmup:
                res["clear"].append(t10[0]); res["hist"].append(t10[1]); res["encode"][op].append(t11[0])
        res.setdefault("stats", {})[op] = [st.exposure, st.white, st.n_lit, st.n_dark]
    # the a-trous call of the same process, on the same frame
    alb, nrm = torch.empty_like(acc), torch.empty_like(acc)
    z = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    den = torch.empty_like(acc)
    torch.cuda.synchronize()
    scene.render_aov_device(wl.camera, prm, tiles, alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), None)
    dp = capi.DenoiseParams(sigma_color=1.0)
    res["denoise"] = []
    for r in range(args.warmup + args.reps):
        scene.denoise_device(W, H, acc.data_ptr(), cnt.data_ptr(), alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), dp, den.data_ptr())
        if r >= args.warmup:
            res["denoise"].append(sum(scene.post_timing(1)))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    env = dict(os.environ)
    env.pop("RGK_LIB", None)

    def child(cmd, what):
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"{what} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    common = ["--workload", args.workload, "--scale", str(args.scale), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    d = child([sys.executable, os.path.abspath(__file__), "--leg", "display"] + common, "the display leg")
    fmt = lambda xs: f"{statistics.median(xs):9.4f}  [{min(xs):9.4f} .. {max(xs):9.4f}]"
    W, H = d["size"]
    P = W * H
    lines = [f"{args.workload} {W}x{H} ({d['geometry']} geometry), an accumulator of one 8 spp round; {args.reps} calls after {args.warmup} warm-up calls per operator, "
             "HIP events on the scene's stream; ms: median [min .. max]"]
    floor = lambda b: b / 8e12 * 1e3
    lines.append(f"  {'clear of the histogram (1028 B)':34s} {fmt(d['clear'])}")
    lines.append(f"  {'k_display_hist':34s} {fmt(d['hist'])}   byte floor {floor(16 * P):.4f} ms ({16 * P / 1e6:.1f} MB at 8 TB/s): x{statistics.median(d['hist']) / floor(16 * P):.1f}")
    for op in OPS:
        xs = d["encode"][op]
        e, w, lit, dark = d["stats"][op]
        lines.append(f"  {'k_display_encode, ' + op:34s} {fmt(xs)}   byte floor {floor(20 * P):.4f} ms ({20 * P / 1e6:.1f} MB at 8 TB/s): x{statistics.median(xs) / floor(20 * P):.1f}"
                     f"   (exposure {e:.4g}, white {w:.4g}; {lit} lit, {dark} black pixels)")
    dn = statistics.median(d["denoise"])
    both = statistics.median(d["hist"]) + statistics.median(d["encode"]["filmic"])
    lines.append(f"  {'rgk_denoise_device, 5 iterations':34s} {fmt(d['denoise'])}   (its launches summed); measure + filmic encode = {both:.4f} ms = {both / dn * 100:.1f} % of it")
    if args.parent_tree:
        parent = os.path.abspath(args.parent_tree)
        rounds = os.path.join(ROOT, "tools", "demod_timing.py")
        plan = [("this tree, plain round", ROOT), ("parent tree, plain round", parent), ("this tree, plain round (again)", ROOT), ("parent tree, plain round (again)", parent)]
        runs = [(name, child([sys.executable, rounds, "--leg", "plain", "--tree", tree] + common, name)) for name, tree in plan]
        first = runs[0][1]
        lines.append(f"the plain round, {args.workload} {first['size'][0]}x{first['size'][1]} x {first['spp']} spp, {args.reps} rounds after {args.warmup} warm-up rounds per leg, each leg "
                     "a process of its own, legs one after the other in one session; wall clock around the entry, ms: median [min .. max]")
        for name, r in runs:
            lines.append(f"  {name:34s} {fmt(r['wall'])}")
        med = lambda r: statistics.median(r["wall"])
        here, parents = [r for n, r in runs if n.startswith("this")], [r for n, r in runs if n.startswith("parent")]
        lo, hi = min(min(r["wall"]) for r in parents), max(max(r["wall"]) for r in parents)
        meds = [med(r) for r in here]
        verdict = ("inside the parent's spread" if all(lo <= m <= hi for m in meds) else
                   "not above it: at or below the parent's fastest round" if all(m <= hi for m in meds) else "ABOVE the parent's spread")
        lines.append(f"  parent's own spread over its two legs: [{lo:.4f} .. {hi:.4f}] ms, medians {', '.join(f'{med(r):.4f}' for r in parents)}; this tree's medians "
                     f"{', '.join(f'{m:.4f}' for m in meds)} -> {verdict}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
