"""What writing one EXR and one PNG costs through the host writers and through the device writers, on one GPU, and that the plain
round did not move.

    python tools/output_timing.py [--workload sponza-1080p] [--scale 1 2] [--reps 20] [--warmup 3] [--dir DIR] [--parent-tree DIR] [--out FILE]

Per scale (1: the workload's own frame, 2: twice its sides) a process of its own: one round at 8 spp for an accumulator with a real
image in it and its display words; then per file kind the host path and the device path ALTERNATE, `reps` repetitions after
`warmup`, wall clock around the call, ms: median [min .. max].  The host path is what render_frame did before the device writers:
the .cpu() copies, rgk_output_normalize and rgk_output_write_exr, or the .cpu() copy and rgk_output_write_png.  Both write to the
same directory (--dir, default a temporary one).  Beside them: the device path's launch times (rgk_scene_get_post_timing 12 and 13)
with their byte floors at 8 TB/s, a device-to-pinned-host copy of the file's size on its own, and a plain write of the same bytes
from memory to the same directory -- the fwrite both paths share.
With --parent-tree (a checkout of the parent commit with its library built): bench.py --gpus 1 once in that tree and once in this
one, one after the other, their ms_per_step side by side."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    """One frame size; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import torch
    from rgk_amd import capi
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import Workload
    wl = Workload(args.workload, scale=args.leg_scale, spp=8)
    scene = rd.Scene(wl.builder.to_desc())
    W, H = wl.xres, wl.yres
    ob = rd.EXRTexture(W, H, torch.device("cuda", 0))
    torch.cuda.synchronize()
    scene.render_round_device(wl.camera, wl.params(), rd.generate_task_list(W, H), ob.data.data_ptr(), ob.count.data_ptr())
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    p = capi.DisplayParams()
    torch.cuda.synchronize()
    st = scene.display_measure_device(W, H, ob.data.data_ptr(), ob.count.data_ptr(), p)
    scene.display_encode_device(W, H, ob.data.data_ptr(), ob.count.data_ptr(), p, st, rgba.data_ptr())
    scene.set_tuning(time_post=1)
    d = args.dir
    paths = {k: os.path.join(d, f"timing_{k}") for k in ("host.exr", "device.exr", "host.png", "device.png", "plain.bin")}
    res = dict(size=[W, H], geometry=wl.geometry, wall={k: [] for k in ("host.exr", "device.exr", "host.png", "device.png")},
               launches={"k_out_max": [], "k_out_pack_exr": [], "k_out_pack_png": [], "k_out_png_sums": []}, copy={}, fwrite={}, bytes={})

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for r in range(args.warmup + args.reps):
        keep = r >= args.warmup
        t = timed(lambda: ob.write(paths["host.exr"], -1.0))
        if keep:
            res["wall"]["host.exr"].append(t)
        t = timed(lambda: ob.write(paths["device.exr"], -1.0, scene))
        if keep:
            res["wall"]["device.exr"].append(t)
            t12 = scene.post_timing(12)
            res["launches"]["k_out_max"].append(t12[0]); res["launches"]["k_out_pack_exr"].append(t12[1])
        t = timed(lambda: rd.write_png(paths["host.png"], rgba))
        if keep:
            res["wall"]["host.png"].append(t)
        t = timed(lambda: rd.write_png_image(paths["device.png"], rgba, scene))
        if keep:
            res["wall"]["device.png"].append(t)
            t13 = scene.post_timing(13)
            res["launches"]["k_out_pack_png"].append(t13[0]); res["launches"]["k_out_png_sums"].append(t13[1])
    for kind in ("exr", "png"):
        host, dev = open(paths[f"host.{kind}"], "rb").read(), open(paths[f"device.{kind}"], "rb").read()
        assert host == dev, f"the {kind} files differ"
        res["bytes"][kind] = len(dev)
        src = torch.zeros(len(dev), dtype=torch.uint8, device="cuda:0")
        pin = torch.empty(len(dev), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        res["copy"][kind], res["fwrite"][kind] = [], []
        for r in range(args.warmup + args.reps):
            def copy():
                pin.copy_(src)
                torch.cuda.synchronize()

            def plain():
                with open(paths["plain.bin"], "wb") as f:
                    f.write(dev)
            tc, tw = timed(copy), timed(plain)
            if r >= args.warmup:
                res["copy"][kind].append(tc); res["fwrite"][kind].append(tw)
    for path in paths.values():
        if os.path.exists(path):
            os.remove(path)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sponza-1080p")
    ap.add_argument("--scale", type=float, nargs="+", default=[1.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg-scale", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg_scale is not None:
        return leg(args)
    env = dict(os.environ)
    env.pop("RGK_LIB", None)

    def child(cmd, what, cwd=None):
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=cwd)
        if r.returncode != 0:
            sys.exit(f"{what} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    fmt = lambda xs: f"{statistics.median(xs):9.3f}  [{min(xs):9.3f} .. {max(xs):9.3f}]"
    med = statistics.median
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        where = os.path.abspath(args.dir) if args.dir else tmp
        os.makedirs(where, exist_ok=True)
        for scale in args.scale:
            d = child([sys.executable, os.path.abspath(__file__), "--leg-scale", str(scale), "--workload", args.workload, "--reps", str(args.reps),
                       "--warmup", str(args.warmup), "--dir", where], f"the leg at scale {scale}")
            W, H = d["size"]
            P = W * H
            lines.append(f"{args.workload} {W}x{H} ({d['geometry']} geometry), an accumulator of one 8 spp round and its display words; host and device path alternating in one "
                         f"process, {args.reps} repetitions after {args.warmup} warm-ups; wall clock around the call, ms: median [min .. max]")
            for kind, host_what in (("exr", ".cpu() + rgk_output_normalize + rgk_output_write_exr"), ("png", ".cpu() + rgk_output_write_png")):
                h, v = d["wall"][f"host.{kind}"], d["wall"][f"device.{kind}"]
                verdict = "device median below host minimum: holds" if med(v) < min(h) else "device median NOT below host minimum"
                lines.append(f"  {kind.upper()} {d['bytes'][kind] / 1e6:6.1f} MB  host   ({host_what})".ljust(86) + fmt(h))
                lines.append(f"  {kind.upper()} {d['bytes'][kind] / 1e6:6.1f} MB  device (rgk_output_write_{kind}_device)".ljust(86) + fmt(v) + f"   x{med(h) / med(v):.1f}; {verdict}")
                lines.append(f"      a device-to-pinned-host copy of the file's bytes on its own".ljust(86) + fmt(d["copy"][kind]))
                lines.append(f"      a plain write of the same bytes from memory (the fwrite both share)".ljust(86) + fmt(d["fwrite"][kind]))
            floor = lambda b: b / 8e12 * 1e3
            floors = {"k_out_max": (16 * P, "12 B + 4 B per pixel read"), "k_out_pack_exr": (16 * P + 8 * P, "16 B per pixel read, 8 B written"),
                      "k_out_pack_png": (4 * P + 3 * P, "4 B per pixel read, 3 B written"), "k_out_png_sums": (6 * P, "the payload read twice")}
            lines.append("  launch times of the device path (HIP events on the scene's stream), ms, with their byte floors at 8 TB/s:")
            for k, xs in d["launches"].items():
                b, what = floors[k]
                lines.append(f"      {k:16s} {fmt(xs)}   byte floor {floor(b):.4f} ms ({b / 1e6:.1f} MB: {what}): x{med(xs) / floor(b):.1f}")
            lines.append(f"      against the copy: EXR launches {med(d['launches']['k_out_max']) + med(d['launches']['k_out_pack_exr']):.3f} ms vs copy {med(d['copy']['exr']):.3f} ms; "
                         f"PNG launches {med(d['launches']['k_out_pack_png']) + med(d['launches']['k_out_png_sums']):.3f} ms vs copy {med(d['copy']['png']):.3f} ms")
    if args.parent_tree:
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "2"]
        runs = [(name, child(cmd, name, cwd=tree)["ms_per_step"]) for name, tree in (("parent tree", os.path.abspath(args.parent_tree)), ("this tree", ROOT))]
        lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup 2 (it does not run the output entries), one run per tree in one session: "
                     + ", ".join(f"{name} {ms:.3f} ms per step" for name, ms in runs)
                     + f"; difference {abs(runs[0][1] - runs[1][1]):.3f} ms (the two parent runs of profiles/post_filter_family.txt differ by 0.332 ms)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
