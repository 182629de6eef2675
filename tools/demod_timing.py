"""What a demodulated round costs, on one GPU.

    python tools/demod_timing.py [--workload sponza-1080p] [--reps 20] [--warmup 3] [--parent-tree DIR] [--out FILE]

The headline workload, one round per repetition on a scene of the process, median [min .. max] of `reps` after `warmup`:
  * a round through rgk_render_round_device -- on this tree and, with --parent-tree (a checkout of the parent commit with its library
    built), on that tree too: each leg runs in a child process of its own (one library per process), the legs alternate
    this / parent / this / parent in one session, and the first pair's spreads say what run-to-run variation is;
  * a round through rgk_render_round_demod_device;
  * the three kernels alone, by HIP events on the scene's stream ("time_post": rgk_scene_get_post_timing 9 and 8).
A round's time is the wall clock around the blocking entry, which queues its passes and waits for them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    """One child: rounds of one kind on the tree in sys.path[0]; prints one JSON line."""
    sys.path.insert(0, args.tree)
    import torch
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import Workload
    wl = Workload(args.workload, scale=args.scale, spp=args.spp)
    scene = rd.Scene(wl.builder.to_desc())
    prm = wl.params()
    W, H = wl.xres, wl.yres
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")
    acc, cnt, dem, div = z(H, W, 3), z(H, W, dt=torch.int32), z(H, W, 3), z(H, W, 3)
    n_tiles = len(rd.generate_task_list(W, H))
    if args.leg == "demod":
        scene.set_tuning(time_post=1)
    wall, k9, k8 = [], [], []
    for r in range(args.warmup + args.reps):
        tiles = rd.generate_task_list(W, H, rd.SEEDSTART, r * n_tiles)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.leg == "demod":
            scene.render_round_demod_device(wl.camera, prm, tiles, acc.data_ptr(), cnt.data_ptr(), dem.data_ptr(), div.data_ptr())
        else:
            scene.render_round_device(wl.camera, prm, tiles, acc.data_ptr(), cnt.data_ptr())
        t1 = time.perf_counter()
        if r < args.warmup:
            continue
        wall.append((t1 - t0) * 1e3)
        if args.leg == "demod":
            k9.append(scene.post_timing(9))
            out = torch.empty_like(dem)
            scene.remodulate_device(W, H, dem.data_ptr(), div.data_ptr(), cnt.data_ptr(), out.data_ptr())
            k8.append(scene.post_timing(8)[0])
    print(json.dumps(dict(leg=args.leg, tree=args.tree, wall=wall, divisor=[t[0] for t in k9], resolve=[t[1] for t in k9], remodulate=k8,
                          size=[W, H], spp=wl.multisample, geometry=wl.geometry, paths=W * H * wl.multisample)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)

    def child(kind, tree):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--tree", tree, "--workload", args.workload, "--scale", str(args.scale), "--reps", str(args.reps),
               "--warmup", str(args.warmup)] + (["--spp", str(args.spp)] if args.spp else [])
        env = dict(os.environ)
        env.pop("RGK_LIB", None)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"leg {kind} on {tree} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    plan = [("this tree, plain round", "plain", ROOT)]
    if args.parent_tree:
        parent = os.path.abspath(args.parent_tree)
        plan += [("parent tree, plain round", "plain", parent), ("this tree, plain round (again)", "plain", ROOT), ("parent tree, plain round (again)", "plain", parent)]
    plan.append(("this tree, demodulated round", "demod", ROOT))
    runs = [(name, child(kind, tree)) for name, kind, tree in plan]
    first = runs[0][1]
    fmt = lambda xs: f"{statistics.median(xs):9.4f}  [{min(xs):9.4f} .. {max(xs):9.4f}]"
    lines = [f"{args.workload} {first['size'][0]}x{first['size'][1]} x {first['spp']} spp ({first['geometry']} geometry, {first['paths'] / 1e6:.1f} M paths per round), {args.reps} rounds "
             f"after {args.warmup} warm-up rounds per leg, each leg a process of its own, legs run one after the other in one session; ms: median [min .. max]",
             f"  {'leg':42s} {'wall clock around the entry':>36s}"]
    for name, r in runs:
        lines.append(f"  {name:42s} {fmt(r['wall']):>36s}")
    med = lambda r: statistics.median(r["wall"])
    d = runs[-1][1]
    plain_here = [r for n, r in runs if n.startswith("this tree, plain")]
    base = statistics.median([med(r) for r in plain_here])
    if args.parent_tree:
        parents = [r for n, r in runs if n.startswith("parent tree")]
        lo, hi = min(min(r["wall"]) for r in parents), max(max(r["wall"]) for r in parents)
        meds = [med(r) for r in plain_here]
        verdict = ("inside the parent's spread" if all(lo <= m <= hi for m in meds) else
                   "not above it: at or below the parent's fastest round" if all(m <= hi for m in meds) else "ABOVE the parent's spread")
        lines.append(f"  parent's own spread over its two legs: [{lo:.4f} .. {hi:.4f}] ms, medians {', '.join(f'{med(r):.4f}' for r in parents)}; this tree's plain medians "
                     f"{', '.join(f'{med(r):.4f}' for r in plain_here)} -> {verdict}")
    lines.append(f"  demodulated round over the plain round of this tree: {med(d) - base:+.4f} ms ({(med(d) / base - 1) * 100:+.2f} %)")
    P = d["paths"]
    pix = d["size"][0] * d["size"][1]
    lines.append("the three kernels alone (HIP events on the scene's stream, per round: summed over the round's passes):")
    for name, xs, byts, what in (("k_demod_divisor", d["divisor"], P * 32, "16 B hit read + 16 B divisor written per path; scene data and the slot's pixel record from the caches"),
                                 ("k_resolve_demod", d["resolve"], P * 32 + pix * 24, "tot and the divisor read per path, two planes += per pixel"),
                                 ("k_remodulate", d["remodulate"], pix * 40, "in, A and the count read, out written per pixel")):
        floor = byts / 8e12 * 1e3
        lines.append(f"  {name:18s} {fmt(xs)}   byte floor {floor:.4f} ms ({byts / 1e6:.1f} MB at 8 TB/s): x{statistics.median(xs) / floor:.1f}   ({what})")
    both = [a + b for a, b in zip(d["divisor"], d["resolve"])]
    lines.append(f"  both round kernels  {fmt(both)}   = {statistics.median(both) / base * 100:.2f} % of a plain round")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
