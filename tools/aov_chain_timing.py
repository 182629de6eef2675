"""HIP-event times of the feature planes that follow mirrors and glass (rgk_render_aov_chain_device), per launch, on one GPU.

    python tools/aov_chain_timing.py [--reps 20] [--warmup 3] [--out FILE]

* Sponza proxy at 1080p, no delta material: the first-hit pass (rgk_render_aov_device) and the chain at max_hops 0 / 4 / 8 in one
  process.  Every queue behind hop 0 is empty there, so what the hops >= 1 cost is launch overhead: two launches per hop.
* Cornell box with spheres at 1024 x 1024, max_hops 8: per hop the queue's length (the pixels whose hops plane says they got
  that far) and the time of its walker and of its k_aov_hop launch.
Times from the scene's "time_post" switch (rgk_scene_get_post_timing, which = 0 / 6): ms, median [min .. max].
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    return f"{statistics.median(xs):8.4f}  [{min(xs):8.4f} .. {max(xs):8.4f}]"


def timed(scene, which, reps, warmup, call):
    rows = []
    for r in range(warmup + reps):
        call()
        if r >= warmup:
            rows.append(scene.post_timing(which))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import SceneFixture, Workload
    lines = [f"{args.reps} repetitions after {args.warmup} warm-up calls; HIP events on the scene's stream, ms: median [min .. max]"]

    def planes(W, H):
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")
        return [new((H, W, 3), torch.float32), new((H, W, 3), torch.float32), new((H, W), torch.float32), new((H, W), torch.int32), new((H, W), torch.uint8)]

    # ---- no delta material: what the empty hops cost
    wl = Workload("sponza-1080p", spp=1)
    scene = rd.Scene(wl.builder.to_desc())
    scene.set_tuning(time_post=1)
    prm, tiles = wl.params(), rd.generate_task_list(wl.xres, wl.yres)
    pl = planes(wl.xres, wl.yres)
    ptr = [p.data_ptr() for p in pl]
    torch.cuda.synchronize()
    lines.append(f"sponza-1080p {wl.xres}x{wl.yres} ({wl.geometry} geometry), no mirror / dielectric / transparent material")
    first = timed(scene, 0, args.reps, args.warmup, lambda: scene.render_aov_device(wl.camera, prm, tiles, *ptr[:4]))
    base = statistics.median(sum(t) for t in first)
    lines.append(f"  first-hit pass (rgk_render_aov_device), all launches   {stat([sum(t) for t in first])}")
    for hops in (0, 4, 8):
        rows = timed(scene, 6, args.reps, args.warmup, lambda: scene.render_aov_chain_device(wl.camera, prm, tiles, hops, *ptr))
        assert int(pl[4].max()) == 0
        total = [sum(t) for t in rows]
        lines.append(f"  chain, max_hops {hops}: all {len(rows[0])} launch intervals          {stat(total)}   vs first-hit pass {statistics.median(total) - base:+.4f}")
        lines.append(f"      hop 0: list + raygen / walker / k_aov_hop          {' / '.join(f'{statistics.median(t[k] for t in rows):.4f}' for k in range(3))}")
        if hops:
            empty = [sum(t[3:]) for t in rows]
            lines.append(f"      hops 1 .. {hops} (empty queues), {2 * hops} launches              {stat(empty)}   = {statistics.median(empty) / (2 * hops) * 1e3:.1f} us per launch")
    del scene

    # ---- delta materials on screen: queue lengths and launch times per hop
    fx = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_cornell-box-spheres.npz"), spp=1)
    scene = rd.Scene(fx.builder.to_desc())
    scene.set_tuning(time_post=1)
    prm, tiles = fx.params(), rd.generate_task_list(fx.xres, fx.yres)
    pl = planes(fx.xres, fx.yres)
    ptr = [p.data_ptr() for p in pl]
    torch.cuda.synchronize()
    rows = timed(scene, 6, args.reps, args.warmup, lambda: scene.render_aov_chain_device(fx.camera, prm, tiles, 8, *ptr))
    first = timed(scene, 0, args.reps, args.warmup, lambda: scene.render_aov_device(fx.camera, prm, tiles, *ptr[:4]))
    hops = pl[4].cpu().numpy()
    lines.append(f"cornell-box-spheres {fx.xres}x{fx.yres}, max_hops 8")
    lines.append(f"  first-hit pass (rgk_render_aov_device), all launches   {stat([sum(t) for t in first])}")
    lines.append(f"  chain, all launches                                    {stat([sum(t) for t in rows])}")
    lines.append(f"  pixel list + ray generation                            {stat([t[0] for t in rows])}")
    for k in range(9):
        lines.append(f"  hop {k}: queue {int((hops >= k).sum()):8d}   walker {stat([t[1 + 2 * k] for t in rows])}   k_aov_hop {stat([t[2 + 2 * k] for t in rows])}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
