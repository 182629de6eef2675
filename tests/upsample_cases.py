"""The inputs of test_gpu_upsample.py, made once and shared: scenes with a full-grid and a low-grid camera, the GPU's own feature
planes of both and a real low-resolution accumulator; the call of rgk_upsample_device on them; and, run as a program, the bit cases
in a process of their own for the RGK_POISON run (python tests/upsample_cases.py --out FILE.npz).

    BIT_CASES      name -> (scene, full size, low size): the cases the kernel is held to the restatement on
    QUALITY_CASES  name -> (scene, full size, low size): the two inputs of the quality test, tools/upsample_sweep.py's too
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from rgk_amd import capi  # noqa: E402
from rgk_amd.config import make_camera, make_params  # noqa: E402
from rgk_amd.workloads import SceneFixture, Workload  # noqa: E402

F = np.float32
# zoo: the material zoo of test_gpu_post.py (mirror, glass, transparent, mixes, an emitter) seen through its 45-degree camera;
# make_camera derives the view rectangle from the sizes it is given, so 61 x 47 and 15 x 11 or 40 x 30 do not share one.
BIT_CASES = {
    "zoo 61x47 from 15x11": ("zoo", (61, 47), (15, 11)),     # ragged workgroups, ratio ~4, different view rectangles
    "zoo 61x47 from 40x30": ("zoo", (61, 47), (40, 30)),     # a ratio that is no integer
    "zoo 61x47 from 61x47": ("zoo", (61, 47), (61, 47)),     # ratio 1
    "spheres 96x96 from 24x24": ("spheres", (96, 96), (24, 24)),
    "zoo 5x3 from 1x1": ("zoo", (5, 3), (1, 1)),             # almost every tap outside the frame
}
# The bit cases run with the definition's starting values, not the shipped ones: every test of the counting rule is live with them.
BIT_PARAMS = dict(plane_tol=0.01, normal_cos=0.9, demodulate=1, albedo_floor=0.02)
QUALITY_CASES = {
    "spheres 96x96 from 24x24": ("spheres", (96, 96), (24, 24)),
    "sponza-proxy 192x108 from 48x27": ("sponza", (192, 108), (48, 27)),
}


class SceneSet:
    """A scene builder with cameras for any grid and the render parameters of its source."""

    def __init__(self, name):
        self.name = name
        if name == "zoo":
            from test_gpu_post import zoo
            self.builder, self.depth, self.bump = zoo(), 4, 1.0
            self._prm = lambda w, h, spp: make_params(w, h, spp, self.depth, bumpscale=self.bump)
            self.camera = lambda w, h: make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=w, yres=h)
        elif name == "spheres":
            wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_cornell-box-spheres.npz"), spp=4)
            c = wl.builder.extra["camera"]
            self.builder = wl.builder
            self.camera = lambda w, h: make_camera(c["pos"], c["lookat"], c["up"], fov=c.get("fov"), focal=c.get("focal"), xres=w, yres=h)
            self._prm = lambda w, h, spp: self._sized(wl.params(), w, h, spp)
        elif name == "sponza":
            wl = Workload("sponza-1080p", scale=0.1, spp=4)
            self.builder = wl.builder

            def cam(w, h):  # as the command line's -p does it: the configuration's camera at the divided sizes
                keep = (wl.cfg.xres, wl.cfg.yres)
                wl.cfg.xres, wl.cfg.yres = w, h
                try:
                    return wl.cfg.get_camera()
                finally:
                    wl.cfg.xres, wl.cfg.yres = keep
            self.camera = cam
            self._prm = lambda w, h, spp: self._sized(wl.params(), w, h, spp)
        else:
            raise KeyError(name)

    @staticmethod
    def _sized(prm, w, h, spp):
        prm.xres, prm.yres, prm.multisample = w, h, spp
        return prm

    def params(self, w, h, spp):
        return self._prm(w, h, spp)

    def cfg(self, w, h, spp):
        """What RenderDriver takes as its configuration."""
        prm = self.params(w, h, spp)

        class Cfg:
            xres, yres, render_rounds, render_minutes = w, h, 1, None
            get_params = staticmethod(lambda sampler=0, flags=0: prm)
        return Cfg


class Inputs:
    """Both grids of one case on a GPU scene `g`: cameras, the feature planes rgk_render_aov makes for them and one round of
    `spp` samples on the low grid (host arrays)."""

    def __init__(self, rd, g, scenes, full, low, spp=4, empty_pixel=True):
        (self.W, self.H), (self.WL, self.HL) = full, low
        self.cam, self.cam_low = scenes.camera(*full), scenes.camera(*low)
        prm_f, prm_l = scenes.params(*full, 1), scenes.params(*low, spp)
        self.albedo, self.normal, self.depth, _ = g.render_aov(self.cam, prm_f, rd.generate_task_list(*full))
        self.low_albedo, self.low_normal, self.low_depth, _ = g.render_aov(self.cam_low, prm_l, rd.generate_task_list(*low))
        self.acc, self.cnt, _ = g.render_round(self.cam_low, prm_l, rd.generate_task_list(*low))
        if empty_pixel and self.WL > 7 and self.HL > 5:
            self.cnt[5, 7] = 0  # a low pixel without samples: never a tap, and 0 as the nearest

    def ref(self, up=None, demodulate=1):
        import upsample_ref as U
        up = up or capi.UpsampleParams(**BIT_PARAMS)
        return U.upsample_ref(self.cam, self.albedo, self.normal, self.depth, self.cam_low, self.acc, self.cnt, self.low_albedo, self.low_normal,
                              self.low_depth, plane_tol=up.plane_tol, normal_cos=up.normal_cos, demodulate=demodulate, albedo_floor=up.albedo_floor)

    def gpu(self, g, up=None, demodulate=1, support=True, poisoned_outputs=False):
        """rgk_upsample_device on device copies -> (out, support or None) as numpy."""
        import torch
        import memstate_ref as M
        up = capi.UpsampleParams.from_buffer_copy(up or capi.UpsampleParams(**BIT_PARAMS))
        up.demodulate = demodulate
        dev = [M.up(a) for a in (self.albedo, self.normal, self.depth, self.acc, self.cnt, self.low_albedo, self.low_normal, self.low_depth)]
        p = [t.data_ptr() for t in dev]
        if not demodulate:
            p[0] = p[5] = None  # the albedo planes may be NULL
        if poisoned_outputs:
            out = M.poisoned_plane(self.H, self.W, 3)
            sup = torch.full((self.H, self.W), 0xFF, dtype=torch.uint8, device="cuda:0") if support else None
        else:
            out = torch.full((self.H, self.W, 3), -1.0, dtype=torch.float32, device="cuda:0")
            sup = torch.full((self.H, self.W), 9, dtype=torch.uint8, device="cuda:0") if support else None
        torch.cuda.synchronize()
        g.upsample_device(self.W, self.H, self.cam, p[0], p[1], p[2], self.WL, self.HL, self.cam_low, p[3], p[4], p[5], p[6], p[7], up, out.data_ptr(),
                          sup.data_ptr() if support else None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), (sup.cpu().numpy() if support else None)


def run_bit_cases(rd, poisoned_outputs=False):
    """Every bit case with demodulate 1 and 0 -> {case: Inputs}, {"case|demodulate": (out, support)}."""
    inputs, results, scenes, gpu_scenes = {}, {}, {}, {}
    for name, (scene, full, low) in BIT_CASES.items():
        if scene not in scenes:
            scenes[scene] = SceneSet(scene)
            gpu_scenes[scene] = rd.Scene(scenes[scene].builder.to_desc())
        inp = Inputs(rd, gpu_scenes[scene], scenes[scene], full, low)
        inputs[name] = inp
        for demodulate in (1, 0):
            results[f"{name}|{demodulate}"] = inp.gpu(gpu_scenes[scene], demodulate=demodulate, poisoned_outputs=poisoned_outputs)
    return inputs, results, gpu_scenes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from rgk_amd import render_driver as rd
    import memstate_ref as M
    inputs, results, _ = run_bit_cases(rd, poisoned_outputs=os.environ.get("RGK_POISON") == "1")
    flat = {"_poisoned_total": np.array([M.poisoned()], np.uint64)}
    for key, (out, sup) in results.items():
        left = int((M.bits(out) == M.POISON_WORD).sum())
        assert left == 0, f"{key}: {left} elements of out were never written"
        flat[f"{key}::out"], flat[f"{key}::support"] = out, sup
    for name, inp in inputs.items():
        flat[f"{name}::acc"], flat[f"{name}::low_depth"] = inp.acc, inp.low_depth
    np.savez(args.out, **flat)
    print("upsample cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
