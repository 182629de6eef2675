"""ORACLE -- test infrastructure only (ctypes wrapper over oracle/librgk_oracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this.
The product (rgk_amd/) never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from rgk_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "librgk_oracle.so")
_p = C.POINTER
_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "all"])
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", HERE, "ref"])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        L = C.CDLL(LIB)
        L.orc_scene_create.restype = C.c_void_p
        L.orc_scene_create.argtypes = [_p(capi.SceneDesc)]
        L.orc_scene_destroy.argtypes = [C.c_void_p]
        L.orc_scene_get_info.argtypes = [C.c_void_p, _p(capi.SceneInfo)]
        L.orc_generate_task_list.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                             C.c_uint32, C.c_uint32, _p(capi.Tile), _p(C.c_uint32)]
        L.orc_render_round.argtypes = [C.c_void_p, _p(capi.Camera), _p(capi.Params), _p(capi.Tile),
                                       C.c_uint32, C.c_void_p, C.c_void_p, _p(capi.Counters), C.c_int]
        L.orc_render_round_split.argtypes = [C.c_void_p, _p(capi.Camera), _p(capi.Params), _p(capi.Tile), C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             _p(C.c_uint64), C.c_void_p, _p(capi.Counters), C.c_int, C.c_int]
        L.orc_trace_closest.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        _p(capi.Counters)]
        L.orc_trace_visibility.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           _p(capi.Counters)]
        L.orc_trace_closest_exhaustive.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_trace_visibility_exhaustive.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_halton_raw.restype = C.c_float
        L.orc_halton_raw.argtypes = [C.c_uint32, C.c_uint32]
        L.orc_sampler_eval.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.orc_bxdf_value.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_bxdf_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, _p(C.c_int)]
        L.orc_texture_sample.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _p(C.c_float), _p(C.c_float)]
        L.orc_libm.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_camera_init.argtypes = [_p(capi.Camera), capi.f3, capi.f3, capi.f3, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float]
        L.orc_camera_ray.argtypes = [_p(capi.Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
        L.orc_test_intersection.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.orc_stratified_sample.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def generate_task_list(xres, yres, seedstart=42, seedcount_base=0, tile_size=32, mid=None):
    L = lib()
    mid = mid or (xres / 2.0, yres / 2.0)
    n = C.c_uint32(0)
    L.orc_generate_task_list(tile_size, xres, yres, mid[0], mid[1], seedstart, seedcount_base, None, C.byref(n))
    tiles = (capi.Tile * n.value)()
    L.orc_generate_task_list(tile_size, xres, yres, mid[0], mid[1], seedstart, seedcount_base, tiles, C.byref(n))
    return tiles


SPLAT_DTYPE = np.dtype([("x", "i4"), ("y", "i4"), ("task", "u4"), ("rgb", "f4", (3,))])


class RoundSplit:
    """What OracleScene.render_round_split returns."""


class OracleScene:
    def __init__(self, desc):
        self.L = lib()
        self.h = self.L.orc_scene_create(C.byref(desc))

    def close(self):
        if self.h:
            self.L.orc_scene_destroy(self.h)
            self.h = None

    __del__ = close

    def info(self):
        i = capi.SceneInfo()
        self.L.orc_scene_get_info(self.h, C.byref(i))
        return i

    def render_round(self, camera, params, tiles, accum=None, count=None, n_threads=0):
        n = len(tiles)
        if accum is None:
            accum = np.zeros((params.yres, params.xres, 3), dtype=np.float32)
            count = np.zeros((params.yres, params.xres), dtype=np.uint32)
        cnt = capi.Counters()
        self.L.orc_render_round(self.h, C.byref(camera), C.byref(params), tiles, n,
                                accum.ctypes.data, count.ctypes.data, C.byref(cnt), n_threads)
        return accum, count, cnt

    def render_round_split(self, camera, params, tiles, want_list=False, exhaustive=False, n_threads=0):
        """render_round's round with its terms kept apart (tests/bdpt_ref.py).  Returns a RoundSplit: `main` float32 (yres, xres, 3),
        the own-pixel sums exactly as render_round adds them; `splat_sum` / `splat_abs` float64 (yres, xres, 3), the sum of the
        splats landing on each pixel and of their absolute values; `splat_n` uint32 (yres, xres), how many landed; `count`;
        `counters`; `lv_kind` (16,) light sub-path vertices by material kind and `lv_none`, the paths whose light sub-path has no
        vertex on a surface; with want_list `splats`, records (x, y, task, rgb) in the order render_round adds them.
        exhaustive: every ray answered by testing every triangle under the walkers' stated rule (trace_closest_exhaustive /
        visibility_exhaustive) instead of the kd-tree: the round the GPU's traversal is pinned to, free of the kd-tree's own
        epsilon-band decisions.  Small scenes only: the cost is rays x triangles."""
        shape = (params.yres, params.xres)
        r = RoundSplit()
        r.main = np.zeros(shape + (3,), np.float32)
        r.splat_sum, r.splat_abs = np.zeros(shape + (3,), np.float64), np.zeros(shape + (3,), np.float64)
        r.splat_n, r.count = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        r.counters = capi.Counters()
        stats = np.zeros(17, np.uint64)
        n, lst = C.c_uint64(0), None
        for _ in range(2 if want_list else 1):          # the second time with room for the list
            if want_list and n.value:
                lst = np.zeros(n.value, SPLAT_DTYPE)
                for a in (r.main, r.splat_sum, r.splat_abs, r.splat_n, r.count):
                    a[...] = 0
            self.L.orc_render_round_split(self.h, C.byref(camera), C.byref(params), tiles, len(tiles), r.main.ctypes.data,
                                          r.splat_sum.ctypes.data, r.splat_abs.ctypes.data, r.splat_n.ctypes.data, r.count.ctypes.data,
                                          None if lst is None else lst.ctypes.data, 0 if lst is None else len(lst), C.byref(n),
                                          stats.ctypes.data, C.byref(r.counters), n_threads, int(exhaustive))
            if not n.value:
                break
        r.n_splats = int(n.value)
        r.lv_kind, r.lv_none = stats[:16].astype(np.int64), int(stats[16])
        if want_list:
            r.splats = lst if lst is not None else np.zeros(0, SPLAT_DTYPE)
        return r

    def trace_closest(self, rays, ignore=None):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        ig = None if ignore is None else np.ascontiguousarray(ignore, dtype=np.int32)
        hits = np.zeros(n, dtype=[("t", "f4"), ("tri", "i4"), ("a", "f4"), ("b", "f4"), ("c", "f4")])
        cnt = capi.Counters()
        self.L.orc_trace_closest(self.h, n, rays.ctypes.data, None if ig is None else ig.ctypes.data,
                                 hits.ctypes.data, C.byref(cnt))
        return hits, cnt

    def visibility(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        vis = np.zeros(len(a), dtype=np.uint8)
        cnt = capi.Counters()
        self.L.orc_trace_visibility(self.h, len(a), a.ctypes.data, b.ctypes.data, vis.ctypes.data, C.byref(cnt))
        return vis, cnt

    def trace_closest_exhaustive(self, rays, ignore=None):
        """trace_closest's layouts, answered by testing every triangle under the walkers' stated rule (Scene::FindExhaustive)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        ig = None if ignore is None else np.ascontiguousarray(ignore, dtype=np.int32)
        hits = np.zeros(n, dtype=[("t", "f4"), ("tri", "i4"), ("a", "f4"), ("b", "f4"), ("c", "f4")])
        self.L.orc_trace_closest_exhaustive(self.h, n, rays.ctypes.data, None if ig is None else ig.ctypes.data, hits.ctypes.data)
        return hits

    def visibility_exhaustive(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        vis = np.zeros(len(a), dtype=np.uint8)
        self.L.orc_trace_visibility_exhaustive(self.h, len(a), a.ctypes.data, b.ctypes.data, vis.ctypes.data)
        return vis


def sampler_eval(seed, index, dim, is2d):
    seed = np.ascontiguousarray(seed, dtype=np.uint32)
    index = np.ascontiguousarray(index, dtype=np.uint32)
    dim = np.ascontiguousarray(dim, dtype=np.uint32)
    out = np.zeros((len(seed), 2), dtype=np.float32)
    lib().orc_sampler_eval(len(seed), seed.ctypes.data, index.ctypes.data, dim.ctypes.data, int(is2d), out.ctypes.data)
    return out
