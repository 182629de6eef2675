"""How much of a preview is a picture: the share of pixels that are 0 or 255 in every channel, per tone curve, beside the image a
user had before the display stage existed.

    python tools/display_quality.py [--spp 32] [--out FILE] [--png-dir DIR]

For the Cornell box and the Sponza proxy at their preview sizes (a quarter of the configured resolution), one round:
  * linear / reinhard / filmic: RenderDriver.display() with the shipped parameters (automatic exposure);
  * normalised only: the accumulator scaled so that its brightest channel is 1 (rgk_output_normalize's automatic scale, what the
    EXR holds) and pushed through the sRGB table alone -- exposure 1, clip at 1.
A pixel that is 0 or 255 in every channel carries no detail; `black` and `white` split that share.  --png-dir keeps the pictures."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--png-dir", default=None)
    args = ap.parse_args()
    import numpy as np
    from rgk_amd import capi
    from rgk_amd import render_driver as rd
    from rgk_amd.workloads import Workload
    lines = [f"share of pixels that are 0 or 255 in every channel (black + white), one round of {args.spp} spp at the preview size; automatic exposure, shipped parameters"]
    for name, wl_name in (("cornell", "cornell-1024"), ("sponza-proxy", "sponza-1080p")):
        wl = Workload(wl_name, scale=0.25, spp=args.spp)
        prm = wl.params()

        class Cfg:
            xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 1, None
            get_params = staticmethod(lambda sampler=0, flags=0: prm)
        scene = rd.Scene(wl.builder.to_desc())
        drv = rd.RenderDriver(scene, Cfg, wl.camera)
        drv.render_round()
        px = drv.total_ob.get_pixels()
        rows = []
        for op in ("linear", "reinhard", "filmic"):
            rgba, st = drv.display(params=capi.DisplayParams(op=capi.DISPLAY_OPS[op]))
            rows.append((op, rgba.cpu().numpy(), f"exposure {st.exposure:.4g}, white {st.white:.4g}, median luminance {st.y_median:.4g}"))
        one = capi.DisplayStats()
        one.exposure, one.white = 1.0, 1.0
        scale = 1.0 / float(px.max())
        rgba, _ = drv.display(image=(px * scale).contiguous(), params=capi.DisplayParams(op=capi.DISPLAY_LINEAR), stats=one)
        rows.append(("normalised only", rgba.cpu().numpy(), f"scale {scale:.4g} (brightest channel {1 / scale:.4g})"))
        lines.append(f"{name} {wl.xres}x{wl.yres}")
        for op, img, note in rows:
            rgb = img[..., :3]
            black, white = float((rgb == 0).all(-1).mean()), float((rgb == 255).all(-1).mean())
            lines.append(f"  {op:16s} {black + white:7.4f}  (black {black:.4f}, white {white:.4f}; mean byte {rgb.mean():6.1f})   {note}")
            if args.png_dir:
                os.makedirs(args.png_dir, exist_ok=True)
                rd.write_png(os.path.join(args.png_dir, f"{name}.{op.replace(' ', '-')}.png"), img)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
