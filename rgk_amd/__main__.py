"""python -m rgk_amd [OPTIONS]... FILE  -- the reference's command line (src/main.cpp:20-260) over the MI355X core.

  -p, --preview     quarter resolution, half the samples (PREVIEW_DIMENTIONS_RATIO 4, PREVIEW_RAYS_RATIO 2); output gets a
                    `.preview` suffix
  -r, --rotate      renders 501 frames rotating the camera around the look-at point (10 s at 50 fps); implies --no-overwrite
  -t, --timed MIN   forces timed mode
  --no-overwrite    skips frames whose output file exists (several machines / processes sharing a directory claim frames this way)
  -s, --scale V     output brightness scale (default: auto, the brightest channel becomes 1)
  -D, --dir DIR     output directory
  -d, --debug X Y   renders only pixel (X, Y) and prints its radiance, sample count and ray counters
  -c, --compare     output gets a `.cmp` suffix (src/main.cpp:129-131,196: an image to put beside an earlier one)
  -v / -q           verbosity up / down (default 2)
  --checkpoint F    raw accumulator checkpoint: resumed from F if it exists, rewritten after every round.  With -r every
                    frame has its own (F gets the frame number as a suffix); a checkpoint written for another scene, camera
                    or parameter set is refused
  --device N        GPU to use (default 0)
  --aov             also writes the first-hit feature images, once per frame: the output name with the suffixes `albedo`,
                    `normal` (world space, as lit) and `depth` (the ray's t in R, G and B; 0 where nothing is hit)
  --denoise         also writes the output name with the suffix `denoised` after every round: the round's image through the
                    feature-guided a-trous filter, normalised with the scale the plain output got.  The plain output is unchanged
  --noise           keeps a second accumulator of the odd rounds (the half-buffer noise estimate): prints the frame's relative noise
                    after every round from the second on, writes the output name with the suffix `noise` -- sqrt of the
                    variance-guided filter's output variance in R, G and B, scaled like the plain output -- after every round that
                    rewrites the output, and makes --denoise use the variance-guided filter from round 2 on.  With --checkpoint
                    the half-buffer is saved beside the checkpoint as `F.half`; resuming a checkpoint that has none is refused
  --until-noise X   implies --noise; stops the frame once the relative noise is <= X (rounds / -t still bound it)
  --adaptive [N]    needs --until-noise: from the second round on a round renders only the 32 x 32 tiles whose own noise is still above
                    their share of the target; every tile is rendered at least N times (default 4, at least 2).  Not with
                    bidirectional rounds ("reverse" > 0)
  --temporal        needs --denoise; for camera animations (-r) over static geometry: after a frame's last round the `denoised` image
                    is written once more from the frame blended into the history the frames before it left -- reprojected through
                    the two cameras, tested against depth, normal and triangle planes -- and then filtered; the blend becomes the
                    next frame's history.  A frame skipped by --no-overwrite or resumed from a checkpoint starts the chain again
                    (the history is not checkpointed).  Not with --noise, --until-noise or --adaptive.  Every other file is unchanged
  --aov-hops K      needs --aov or --denoise; K = 0 .. 8 (default 0: off).  The feature planes follow up to K mirror, glass and
                    transparent surfaces along the path the integrator takes and describe the first other surface seen through
                    them (depth: the length of the whole chain; albedo: times the surfaces' colours): --aov writes those planes
                    and, beside them, the suffix `hops` (the surfaces passed, in R, G and B), --denoise filters with them.  Not
                    with --temporal.  The plain output is unchanged
  --upsample        needs -p: after every round that rewrites the output, also writes the output name with the suffix `upsampled` at
                    the configuration's FULL resolution -- the quarter-resolution accumulator reconstructed on the full grid,
                    guided by the normal and depth planes of both grids (one extra ray per full-resolution pixel, once): a pixel
                    takes radiance only from quarter-resolution pixels on its own surface; scaled like the plain output.  With --denoise the upsampled image
                    is filtered at full resolution; the `denoised` file stays the quarter-resolution one.  Not with --temporal,
                    --noise, --until-noise, --adaptive, --aov-hops or -d.  Every other file is unchanged
  --demod           needs --denoise or --upsample: rounds also accumulate each sample's radiance over the albedo at the first hit of the
                    sample's own camera ray (floored at 0.02) and the sum of those divisors.  The `denoised` image is then that
                    irradiance filtered without the centre-ray division and multiplied by the pixel's mean divisor; the `upsampled`
                    image is the quarter-resolution irradiance reconstructed (and, with --denoise, filtered) on the full grid and
                    multiplied by the full-resolution albedo.  Also writes the suffix `irradiance`, scaled like the plain output,
                    after every round that rewrites the output.  With --checkpoint the two sums are saved beside it as `F.demod`
                    and `F.div`; resuming a checkpoint that has none is refused.  Not with --noise, --until-noise, --adaptive,
                    --temporal, --aov-hops, -d or bidirectional rounds ("reverse" > 0).  Without the switch every file is unchanged
  --png [OP]        also writes a picture a viewer can show: beside the output and, with --denoise and --upsample, beside the `denoised`
                    and `upsampled` files, an 8-bit sRGB PNG of the same stem after every round that rewrites them.  Made from the
                    image before its brightness scale: automatic exposure (the median luminance of the lit pixels goes to 0.18),
                    the tone curve OP = linear (clip at 1), reinhard (luminance, white point at the 99.5th percentile) or filmic
                    (default; per channel), then the sRGB transfer function.  Exposure and white point are measured on the
                    accumulator and shared by the pictures of a round, per frame under -r.  Give FILE first, or write --png=OP.
                    Not with -d.  Without the switch every file is unchanged
  --exposure EV     needs --png: a fixed exposure scale of 2^EV (-100 .. 100) instead of the automatic one
  --host-output     assemble every EXR and PNG on the host from downloaded copies, as before the device writers
                    (rgk_output_write_exr_device / rgk_output_write_png_device) existed; the files are byte-identical either way
FILE is a .json or .rtc scene config.  One process drives one GPU; several GPUs: python -m torch.distributed.run ... bench.py.
"""
import argparse
import os
import sys

from . import capi
from . import render_driver as rd
from .config import ConfigFileException, load_config
from .monitor import FrameMonitor, format_int5, format_percent

PREVIEW_DIMENSIONS_RATIO, PREVIEW_RAYS_RATIO = 4, 2  # src/global_config.hpp:10-11


def insert_file_suffix(path, suffix):
    """Utils::InsertFileSuffix (src/utils.cpp:79-82)."""
    name, ext = os.path.splitext(path)
    return f"{name}.{suffix}{ext}" if ext else f"{path}.{suffix}."


def frame_digest(sb, camera, params):
    """64-bit digest of what a frame is rendered from: geometry, materials, textures, lights, sky, camera and the PathTracer
    parameters.  Rides in the checkpoint header (rgk_accum_set_tag): resuming after any of them changed would silently mix
    two different images in one accumulator."""
    import hashlib
    h = hashlib.blake2b(digest_size=8)
    sb.finalize()
    for a in (sb.V, sb.N, sb.T, sb.UV, sb.F, sb.FM):
        if a is not None:
            h.update(a.tobytes())
    h.update(repr([(sorted(m.items())) for m in sb.materials]).encode())
    for t in sb.textures:
        h.update(repr((t["kind"], t.get("color"))).encode())
        for key in ("data", "lut"):
            if t.get(key) is not None:
                h.update(t[key].tobytes())
    h.update(repr((sb.pointlights, [list(a) for a in sb.areal], sorted((k, str(v)) for k, v in sb.sky.items()))).encode())
    h.update(bytes(camera))  # ctypes structures: their bytes
    h.update(bytes(params))
    return int.from_bytes(h.digest(), "little") or 1


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m rgk_amd", add_help=True, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("-p", "--preview", action="store_true")
    ap.add_argument("-r", "--rotate", action="store_true")
    ap.add_argument("-t", "--timed", type=int, default=None)
    ap.add_argument("--no-overwrite", action="store_true")
    ap.add_argument("-s", "--scale", type=float, default=None)
    ap.add_argument("-D", "--dir", default="")
    ap.add_argument("-d", "--debug", nargs=2, type=int, metavar=("X", "Y"))
    ap.add_argument("-c", "--compare", action="store_true")
    ap.add_argument("-v", action="count", default=0)
    ap.add_argument("-q", action="count", default=0)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--aov", action="store_true")
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--until-noise", type=float, default=None, metavar="X")
    ap.add_argument("--adaptive", type=int, nargs="?", const=4, default=None, metavar="MIN_VISITS")
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--frames", type=int, default=None, help="with -r: stop after this many frames (default: all 501)")
    ap.add_argument("--aov-hops", type=int, default=None, metavar="K")
    ap.add_argument("--upsample", action="store_true")
    ap.add_argument("--demod", action="store_true")
    ap.add_argument("--png", nargs="?", const="filmic", default=None, choices=sorted(capi.DISPLAY_OPS), metavar="OP")
    ap.add_argument("--exposure", type=float, default=None, metavar="EV")
    ap.add_argument("--host-output", action="store_true")
    args = ap.parse_args(argv)
    verbosity = max(0, 2 + args.v - args.q)
    say = lambda lvl, *a: print(*a) if verbosity >= lvl else None
    if args.adaptive is not None and (args.until_noise is None or args.adaptive < 2):
        print("ERROR: --adaptive needs --until-noise." if args.until_noise is None else "ERROR: Invalid argument for --adaptive (at least 2).")
        return 1
    if args.temporal and (not args.denoise or args.noise or args.until_noise is not None or args.adaptive is not None):
        print("ERROR: --temporal needs --denoise." if not args.denoise else "ERROR: --temporal cannot be combined with --noise, --until-noise or --adaptive.")
        return 1
    if args.aov_hops is not None:
        if not 0 <= args.aov_hops <= capi.AOV_MAX_HOPS:
            print(f"ERROR: Invalid argument for --aov-hops (0 to {capi.AOV_MAX_HOPS}).")
            return 1
        if not (args.aov or args.denoise):
            print("ERROR: --aov-hops needs --aov or --denoise.")
            return 1
        if args.temporal:
            print("ERROR: --aov-hops cannot be combined with --temporal.")
            return 1
    aov_hops = args.aov_hops or 0
    if args.upsample:
        if not args.preview:
            print("ERROR: --upsample needs -p (--preview).")
            return 1
        clash = [name for name, on in (("--temporal", args.temporal), ("--noise", args.noise), ("--until-noise", args.until_noise is not None),
                                       ("--adaptive", args.adaptive is not None), ("--aov-hops", args.aov_hops is not None), ("-d", args.debug is not None)) if on]
        if clash:
            print(f"ERROR: --upsample cannot be combined with {clash[0]}.")
            return 1
    if args.demod:
        if not (args.denoise or args.upsample):
            print("ERROR: --demod needs --denoise or --upsample.")
            return 1
        clash = [name for name, on in (("--noise", args.noise), ("--until-noise", args.until_noise is not None), ("--adaptive", args.adaptive is not None),
                                       ("--temporal", args.temporal), ("--aov-hops", args.aov_hops is not None), ("-d", args.debug is not None)) if on]
        if clash:
            print(f"ERROR: --demod cannot be combined with {clash[0]}.")
            return 1
    display = None
    if args.exposure is not None and (args.png is None or not -100.0 <= args.exposure <= 100.0):  # (false for NaN)
        print("ERROR: --exposure needs --png." if args.png is None else "ERROR: Invalid argument for --exposure (-100 to 100).")
        return 1
    if args.png is not None:
        if args.debug is not None:
            print("ERROR: --png cannot be combined with -d.")
            return 1
        display = capi.DisplayParams(op=capi.DISPLAY_OPS[args.png], exposure=2.0 ** args.exposure if args.exposure is not None else 0.0)
    try:
        cfg = load_config(args.file)
    except ConfigFileException as e:
        print("Failed to load config file:", e)
        return 1
    if args.demod and int(getattr(cfg, "reverse", 0)) > 0:
        print('ERROR: --demod cannot be combined with bidirectional rounds ("reverse" > 0 in the configuration).')
        return 1
    if args.timed is not None:
        if args.timed <= 0:
            print("ERROR: Invalid argument for -t (--time).")
            return 1
        cfg.render_minutes, cfg.render_rounds = args.timed, 1
    if args.scale is not None:
        cfg.output_scale = args.scale
    track_noise = args.noise or args.until_noise is not None
    if args.until_noise is not None and not args.until_noise > 0:
        print("ERROR: Invalid argument for --until-noise.")
        return 1
    if args.demod and not args.rotate and args.checkpoint and os.path.exists(args.checkpoint):
        for suffix in (".demod", ".div"):
            if not os.path.exists(args.checkpoint + suffix):
                print(f"ERROR: cannot resume from `{args.checkpoint}`: {rd.missing_demod_message(args.checkpoint, suffix)}")  # (before the scene is built and a GPU is asked for)
                return 1
    if track_noise and not args.rotate and args.checkpoint and os.path.exists(args.checkpoint) and not os.path.exists(args.checkpoint + ".half"):
        print(f"ERROR: cannot resume from `{args.checkpoint}`: {rd.missing_half_message(args.checkpoint)}")  # (before the scene is built and a GPU is asked for)
        return 1
    output_file = os.path.join(args.dir, cfg.output_file) if args.dir else cfg.output_file
    if args.preview:
        output_file = insert_file_suffix(output_file, "preview")
    if args.compare:
        output_file = insert_file_suffix(output_file, "cmp")  # main.cpp:196 (after the preview suffix, before the frame number)
    full_res = (cfg.xres, cfg.yres)  # --upsample: the grid the preview is reconstructed on
    if args.preview:
        cfg.xres //= PREVIEW_DIMENSIONS_RATIO
        cfg.yres //= PREVIEW_DIMENSIONS_RATIO
        cfg.multisample = max(1, cfg.multisample // PREVIEW_RAYS_RATIO)
    try:
        sb = cfg.build_scene(asset_dir=os.environ.get("RGK_ASSET_DIR"))
    except (ConfigFileException, RuntimeError) as e:
        print("Failed to load data from config file:", e)
        return 1
    cfg.get_camera(0.0)  # main.cpp:221: the camera is read before the post-check, so its keys count as used
    for w in cfg.perform_post_check():
        say(1, w if w.startswith("WARNING") else f'WARNING: Unused key "{w}" in the config file.')
    import torch
    scene = rd.Scene(sb.to_desc(), device=args.device)
    device = torch.device("cuda", args.device)
    no_overwrite = args.no_overwrite or args.rotate
    fps, time_length = 50.0, (10.0 if args.rotate else 0.0)
    n_frames = int(time_length * fps) + 1
    history = rd.TemporalHistory() if args.temporal else None  # one chain across the frames of -r
    for frame_no in range(n_frames if args.frames is None else min(n_frames, args.frames)):
        t = frame_no / fps
        out = insert_file_suffix(output_file, format_int5(frame_no)) if args.rotate else output_file
        if no_overwrite and os.path.exists(out):
            say(1, f"File `{out}` exists, not overwriting.")
            if history is not None:
                history.reset()  # its frame is not rendered here: the chain starts again
            continue
        if args.rotate:
            open(out, "ab").close()  # claim the frame before rendering it (processes sharing the directory skip it)
            say(1, f"Rendering frame #{frame_no} of ~{int(time_length * fps)} ({format_percent(t / time_length * 100.0)})")
        camera = cfg.get_camera(t / time_length if args.rotate else 0.0)
        upsample_to = None
        if args.upsample:  # the frame's camera as the configuration has it before -p divides its sizes
            low_res = (cfg.xres, cfg.yres)
            cfg.xres, cfg.yres = full_res
            upsample_to = (cfg.get_camera(t / time_length if args.rotate else 0.0),) + full_res
            cfg.xres, cfg.yres = low_res
        try:
            drv = rd.RenderDriver(scene, cfg, camera, device=device, track_noise=track_noise,
                                  adaptive=capi.AdaptParams(args.until_noise, args.adaptive) if args.adaptive is not None else None, history=history,
                                  aov_hops=aov_hops, device_output=not args.host_output, **(dict(track_demod=True) if args.demod else {}))
        except ValueError as e:
            print(f"ERROR: {e}")
            return 1
        if args.debug:
            x, y = args.debug
            if not (0 <= x < cfg.xres and 0 <= y < cfg.yres):
                print("ERROR: debug pixel outside the frame")
                return 1
            tile = (capi.Tile * 1)()
            # the pixel as its own 1 x 1 task with the seed RenderPixel would give it inside its 32 x 32 tile of round 0
            tiles = rd.generate_task_list(cfg.xres, cfg.yres, rd.SEEDSTART, 0)
            home = next(tl for tl in tiles if tl.x0 <= x < tl.x1 and tl.y0 <= y < tl.y1)
            k = (y - home.y0) * (home.x1 - home.x0) + (x - home.x0)
            tile[0].x0, tile[0].x1, tile[0].y0, tile[0].y1 = x, x + 1, y, y + 1
            tile[0].seed = (home.seed + k * 0x42424242) & 0xFFFFFFFF
            acc, cnt, c = scene.render_round(camera, drv.params, tile)
            px = acc[y, x] / max(1, int(cnt[y, x]))
            print(f"pixel ({x}, {y}): radiance {px[0]:.9g} {px[1]:.9g} {px[2]:.9g}  samples {int(cnt[y, x])}  path rays {c.path_rays}  shadow rays {c.shadow_rays}")
            return 0
        # one checkpoint per frame (a finished frame's checkpoint says "all rounds done": the next frame, seen from another
        # camera, would render nothing on top of it), tagged with what the frame is rendered from
        ckpt = (insert_file_suffix(args.checkpoint, format_int5(frame_no)) if args.rotate else args.checkpoint) if args.checkpoint else None
        drv.checkpoint_tag = frame_digest(sb, camera, drv.params)
        if ckpt and os.path.exists(ckpt):
            try:
                drv.load_checkpoint(ckpt)
            except RuntimeError as e:
                print(f"ERROR: cannot resume from `{ckpt}`: {e}")
                return 1
            say(2, f"Resumed from `{ckpt}`: {drv.rounds_done} rounds done.")
            if history is not None:
                history.reset()  # the history is not checkpointed: a resumed frame starts its chain again
        say(2, f"Writing to file {out}")
        timed = cfg.render_minutes is not None
        with FrameMonitor(scene, timed, cfg.render_rounds, cfg.render_minutes or 0, cfg.xres * cfg.yres, verbosity=verbosity) as mon:
            drv.render_frame(rounds=max(0, cfg.render_rounds - drv.rounds_done) if not timed else None, output_file=out, checkpoint=ckpt,
                             aov_files={k: insert_file_suffix(out, k) for k in ("albedo", "normal", "depth") + (("hops",) if aov_hops > 0 else ())} if args.aov else None,
                             denoised_file=insert_file_suffix(out, "denoised") if args.denoise else None, temporal=args.temporal,
                             **(dict(upsampled_file=insert_file_suffix(out, "upsampled"), upsample_to=upsample_to) if args.upsample else {}),
                             **(dict(irradiance_file=insert_file_suffix(out, "irradiance")) if args.demod else {}),
                             **(dict(display=display) if display is not None else {}),
                             **(dict(until_noise=args.until_noise, noise_file=insert_file_suffix(out, "noise"),
                                     on_noise=lambda r, rel, n_live=None: say(1, f"Round {r}: " + (f"{n_live} live tiles, " if n_live is not None else "") +
                                                                                  f"relative noise {rel:.4g}")) if track_noise else {}))
            mon.rays_done = sum(c.path_rays for c in drv.counters)
        if display is not None and drv.display_stats is not None:
            st = drv.display_stats
            say(2, f"Display: exposure {st.exposure:.9g} white {st.white:.9g} (median luminance {st.y_median:.9g}, {st.n_lit} lit and {st.n_dark} black pixels)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
