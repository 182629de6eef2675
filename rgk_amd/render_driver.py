"""Host-side mirror of the reference's render driver, over the C ABI.

Mirrors (names, argument meaning, behaviour) reference src/render_driver.cpp:
  GenerateTaskList :30-46, RenderDriver::RenderRound :144-190, RenderDriver::RenderFrame
  :192-253 (rounds mode and timed mode), and EXRTexture's accumulator half
  (src/texture.cpp:342-354,376-412: AddPixel / GetPixel / Normalize / Accumulate).

The reference runs tiles on a CPU thread pool inside one process.  Here the per-task
body runs on the GPU behind `rgk_render_round*`; with world_size > 1 (one process per
GPU, torch.distributed) tile i of the centre-out list goes to rank i % world_size and
the per-GPU private accumulators are summed with one reduce per round
(EXRTexture::Accumulate under the mutex, render_driver.cpp:179-182, becomes the RCCL
reduce).  Seeds depend only on (round, tile index, pixel-in-tile): the image does not
depend on the number of GPUs.
"""
import ctypes as C
import itertools
import time

import numpy as np

from . import capi

TILE_SIZE = 32  # src/global_config.hpp:8
SEEDSTART = 42  # src/render_driver.cpp:222
# The denoiser's default sigma_color is DENOISE_SIGMA_K x the mean over pixels of the largest channel of the image: the k that
# minimises the summed relative L2 error of the CPU sweep in DESIGN.md ("Feature buffers and the a-trous denoiser";
# tools/denoise_sweep.py reproduces it).
DENOISE_SIGMA_K = 6.0
# rgk_noise_tile: the per-tile sums of rgk_noise_estimate_device, which rgk_adapt_select reads
NOISE_TILE_DTYPE = np.dtype([("sum_var", "f8"), ("sum_sq", "f8"), ("n_estimable", "u8")])


def tile_grid(xres, yres, tile_size=TILE_SIZE):
    """(tiles_y, tiles_x) of a frame; in the row-major order of noise()["tiles"] a tile is (y0 // tile_size) * tiles_x + x0 // tile_size."""
    return -(-yres // tile_size), -(-xres // tile_size)


def generate_task_list(xres, yres, seedstart=SEEDSTART, seedcount_base=0, tile_size=TILE_SIZE, mid=None):
    """GenerateTaskList + the `seedstart + c` each task's PathTracer gets."""
    lib = capi.load_product()
    mid = mid or (xres / 2.0, yres / 2.0)
    n = C.c_uint32(0)
    capi.check(lib, lib.rgk_generate_task_list(tile_size, xres, yres, mid[0], mid[1], seedstart, seedcount_base, None, C.byref(n)))
    tiles = (capi.Tile * n.value)()
    capi.check(lib, lib.rgk_generate_task_list(tile_size, xres, yres, mid[0], mid[1], seedstart, seedcount_base, tiles, C.byref(n)))
    return tiles


def shard_tiles(tiles, rank, world_size):
    """Round-robin deal of the centre-out list: tile i -> rank i % world_size (rgk_shard_tiles)."""
    lib = capi.load_product()
    n = C.c_uint32(0)
    capi.check(lib, lib.rgk_shard_tiles(tiles, len(tiles), rank, world_size, None, C.byref(n)))
    out = (capi.Tile * n.value)()
    capi.check(lib, lib.rgk_shard_tiles(tiles, len(tiles), rank, world_size, out, C.byref(n)))
    return out


class Scene:
    """Device-resident committed scene (rgk_scene_create)."""

    def __init__(self, builder_or_desc, device=0):
        self.lib = capi.load_product()
        self._builder = builder_or_desc if hasattr(builder_or_desc, "to_desc") else None
        desc = builder_or_desc.to_desc() if self._builder is not None else builder_or_desc
        h = C.c_void_p()
        capi.check(self.lib, self.lib.rgk_scene_create(C.byref(desc), device, C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgk_scene_destroy(self.h)
            self.h = None

    __del__ = close

    def set_tuning(self, **kw):
        """rgk_scene_set_tuning: per-scene tuning switches (entry_points, entry_cap, light_entry, sample_group, batch_paths,
        workspace_gb, beam, const_light, last_vertex); none changes a result.

        last_vertex (default 1): the last bounce of a unidirectional pass is shaded by k_last_vertex; 0: by k_shade.

        const_light (default 1): where info().const_light == 1 -- one point light of size 0, nothing else that emits, no -0.0 in
        its position, and the light pick's own float comparisons select it for the largest sample 1 - 2^-24 -- unidirectional
        rounds take the light as launch constants instead of sampling, storing and re-reading it per path, and queue 32-byte
        shadow records without the shared origin.  Exact: the pick has one outcome, and pos + 0 * v == pos.  0: per-path route."""
        for k, v in kw.items():
            capi.check(self.lib, self.lib.rgk_scene_set_tuning(self.h, k.encode(), float(v)))
        return self

    def refit(self, vertices, normals=None, tangents=None):
        """rgk_scene_refit: moved vertices, same triangles -- records, epsilon, box, light tables recomputed, the tree refit."""
        arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (vertices, normals, tangents)]
        capi.check(self.lib, self.lib.rgk_scene_refit(self.h, *[None if a is None else a.ctypes.data for a in arr]))
        return self

    def info(self):
        i = capi.SceneInfo()
        capi.check(self.lib, self.lib.rgk_scene_get_info(self.h, C.byref(i)))
        return i

    def trace_closest(self, rays, ignore=None, count=False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        ig = None if ignore is None else np.ascontiguousarray(ignore, dtype=np.int32)
        hits = np.zeros(n, dtype=[("t", "f4"), ("tri", "i4"), ("a", "f4"), ("b", "f4"), ("c", "f4")])
        cnt = capi.Counters()
        capi.check(self.lib, self.lib.rgk_trace_closest(self.h, n, rays.ctypes.data, None if ig is None else ig.ctypes.data,
                                                        hits.ctypes.data, C.byref(cnt) if count else None))
        return hits, cnt

    def visibility(self, a, b, count=False):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        vis = np.zeros(len(a), dtype=np.uint8)
        cnt = capi.Counters()
        capi.check(self.lib, self.lib.rgk_trace_visibility(self.h, len(a), a.ctypes.data, b.ctypes.data, vis.ctypes.data,
                                                           C.byref(cnt) if count else None))
        return vis, cnt

    def render_round(self, camera, params, tiles, accum=None, count=None):
        """Host-buffer entry point: accum (yres, xres, 3) float32 +=, count (yres, xres) uint32 +=."""
        if accum is None:
            accum = np.zeros((params.yres, params.xres, 3), dtype=np.float32)
            count = np.zeros((params.yres, params.xres), dtype=np.uint32)
        cnt = capi.Counters()
        capi.check(self.lib, self.lib.rgk_render_round(self.h, C.byref(camera), C.byref(params), tiles, len(tiles),
                                                       accum.ctypes.data, count.ctypes.data, C.byref(cnt)))
        return accum, count, cnt

    def render_aov(self, camera, params, tiles, albedo=None, normal=None, depth=None, tri=None, sentinel=None):
        """rgk_render_aov, host buffers: first-hit albedo / normal (y, x, 3) float32, depth (y, x) float32 and triangle id
        (y, x) int32 of the tiles' pixels.  Planes that are not passed in are created (filled with `sentinel`, default 0)."""
        y, x = params.yres, params.xres
        fill = 0 if sentinel is None else sentinel
        albedo = np.full((y, x, 3), fill, np.float32) if albedo is None else albedo
        normal = np.full((y, x, 3), fill, np.float32) if normal is None else normal
        depth = np.full((y, x), fill, np.float32) if depth is None else depth
        tri = np.full((y, x), fill, np.int32) if tri is None else tri
        capi.check(self.lib, self.lib.rgk_render_aov(self.h, C.byref(camera), C.byref(params), tiles, len(tiles), albedo.ctypes.data,
                                                     normal.ctypes.data, depth.ctypes.data, tri.ctypes.data))
        return albedo, normal, depth, tri

    def render_aov_device(self, camera, params, tiles, d_albedo=None, d_normal=None, d_depth=None, d_tri=None):
        """rgk_render_aov_device: DEVICE pointers (ints) on the scene's GPU; any may be None."""
        capi.check(self.lib, self.lib.rgk_render_aov_device(self.h, C.byref(camera), C.byref(params), tiles, len(tiles),
                                                            d_albedo, d_normal, d_depth, d_tri))

    def render_aov_chain(self, camera, params, tiles, max_hops, albedo=None, normal=None, depth=None, tri=None, hops=None, sentinel=None):
        """rgk_render_aov_chain, host buffers: the planes of render_aov, followed through up to `max_hops` mirror / dielectric /
        transparent surfaces to the first other surface, and hops (y, x) uint8, the delta surfaces passed on the way.  Planes that
        are not passed in are created (filled with `sentinel`, default 0)."""
        y, x = params.yres, params.xres
        fill = 0 if sentinel is None else sentinel
        albedo = np.full((y, x, 3), fill, np.float32) if albedo is None else albedo
        normal = np.full((y, x, 3), fill, np.float32) if normal is None else normal
        depth = np.full((y, x), fill, np.float32) if depth is None else depth
        tri = np.full((y, x), fill, np.int32) if tri is None else tri
        hops = np.full((y, x), fill, np.uint8) if hops is None else hops
        capi.check(self.lib, self.lib.rgk_render_aov_chain(self.h, C.byref(camera), C.byref(params), tiles, len(tiles), max_hops, albedo.ctypes.data,
                                                           normal.ctypes.data, depth.ctypes.data, tri.ctypes.data, hops.ctypes.data))
        return albedo, normal, depth, tri, hops

    def render_aov_chain_device(self, camera, params, tiles, max_hops, d_albedo=None, d_normal=None, d_depth=None, d_tri=None, d_hops=None):
        """rgk_render_aov_chain_device: DEVICE pointers (ints) on the scene's GPU; any may be None."""
        capi.check(self.lib, self.lib.rgk_render_aov_chain_device(self.h, C.byref(camera), C.byref(params), tiles, len(tiles), max_hops,
                                                                  d_albedo, d_normal, d_depth, d_tri, d_hops))

    def denoise_device(self, xres, yres, d_accum_rgb, d_accum_count, d_albedo, d_normal, d_depth, params, d_out_rgb):
        """rgk_denoise_device: the guided a-trous filter of a whole frame, DEVICE pointers (ints) on the scene's GPU."""
        capi.check(self.lib, self.lib.rgk_denoise_device(self.h, xres, yres, d_accum_rgb, d_accum_count, d_albedo, d_normal, d_depth,
                                                         C.byref(params), d_out_rgb))

    def noise_estimate_device(self, xres, yres, tile_size, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, d_variance=None):
        """rgk_noise_estimate_device: DEVICE pointers (ints) on the scene's GPU -> a (tiles_y, tiles_x) structured array with the
        fields sum_var, sum_sq (float64) and n_estimable (uint64)."""
        ty, tx = tile_grid(xres, yres, tile_size)
        tiles = (capi.NoiseTile * (ty * tx))()
        capi.check(self.lib, self.lib.rgk_noise_estimate_device(self.h, xres, yres, tile_size, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count,
                                                                tiles, d_variance))
        return np.frombuffer(tiles, dtype=NOISE_TILE_DTYPE).reshape(ty, tx).copy()

    def denoise_variance_device(self, xres, yres, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, d_albedo, d_normal, d_depth, params,
                                d_out_rgb, d_out_variance=None):
        """rgk_denoise_variance_device: the variance-guided a-trous filter of a whole frame, DEVICE pointers (ints)."""
        capi.check(self.lib, self.lib.rgk_denoise_variance_device(self.h, xres, yres, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, d_albedo,
                                                                  d_normal, d_depth, C.byref(params), d_out_rgb, d_out_variance))

    def round_fold_device(self, xres, yres, tiles, to_half, d_round_rgb, d_round_count, d_total_rgb, d_total_count, d_half_rgb, d_half_count):
        """rgk_round_fold_device: total += round, half += round where to_half[i], round = 0 over the listed tiles' pixels and nowhere
        else; DEVICE pointers (ints) on the scene's GPU, to_half one flag per tile."""
        flags = np.ascontiguousarray(to_half, dtype=np.uint8)
        assert flags.shape == (len(tiles),)
        capi.check(self.lib, self.lib.rgk_round_fold_device(self.h, xres, yres, tiles, len(tiles), flags.ctypes.data, d_round_rgb, d_round_count,
                                                            d_total_rgb, d_total_count, d_half_rgb, d_half_count))

    def temporal_reproject_device(self, xres, yres, cam_cur, cam_prev, d_depth_cur, d_normal_cur, d_tri_cur, d_depth_prev, d_normal_prev, d_tri_prev,
                                  d_hist_rgb_prev, d_hist_len_prev, params, d_hist_rgb, d_hist_len):
        """rgk_temporal_reproject_device: the previous frame's history carried to the current frame's pixels; DEVICE pointers (ints)
        on the scene's GPU, params a capi.TemporalParams (its ranges are checked here first: ValueError)."""
        params.check()
        capi.check(self.lib, self.lib.rgk_temporal_reproject_device(self.h, xres, yres, C.byref(cam_cur), C.byref(cam_prev), d_depth_cur, d_normal_cur,
                                                                    d_tri_cur, d_depth_prev, d_normal_prev, d_tri_prev, d_hist_rgb_prev, d_hist_len_prev,
                                                                    C.byref(params), d_hist_rgb, d_hist_len))

    def temporal_blend_device(self, xres, yres, d_accum_rgb, d_accum_count, d_albedo, d_hist_rgb, d_hist_len, params, d_out_hist_rgb, d_out_hist_len,
                              d_out_rgb):
        """rgk_temporal_blend_device: the accumulator's image blended into the reprojected history -> the next frame's history
        (demodulated) and the image to filter; DEVICE pointers (ints), d_albedo may be None without demodulation."""
        params.check()
        capi.check(self.lib, self.lib.rgk_temporal_blend_device(self.h, xres, yres, d_accum_rgb, d_accum_count, d_albedo, d_hist_rgb, d_hist_len,
                                                                C.byref(params), d_out_hist_rgb, d_out_hist_len, d_out_rgb))

    def upsample_device(self, xres, yres, cam, d_albedo, d_normal, d_depth, xl, yl, cam_low, d_low_accum_rgb, d_low_accum_count, d_low_albedo,
                        d_low_normal, d_low_depth, params, d_out_rgb, d_out_support=None):
        """rgk_upsample_device: a low-resolution accumulator (xl x yl, cam_low) reconstructed on the xres x yres grid of `cam`, guided
        by the feature planes of both grids; DEVICE pointers (ints) on the scene's GPU, params a capi.UpsampleParams (its ranges
        are checked here first: ValueError).  The albedo planes may be None without demodulation, d_out_support (P bytes: 1 ring 1,
        2 ring 2, 0 nearest or outside) too."""
        params.check()
        capi.check(self.lib, self.lib.rgk_upsample_device(self.h, xres, yres, C.byref(cam), d_albedo, d_normal, d_depth, xl, yl, C.byref(cam_low),
                                                          d_low_accum_rgb, d_low_accum_count, d_low_albedo, d_low_normal, d_low_depth, C.byref(params),
                                                          d_out_rgb, d_out_support))

    def render_round_demod_device(self, camera, params, tiles, d_accum_ptr, d_count_ptr, d_demod_ptr, d_div_ptr, albedo_floor=capi.DEMOD_ALBEDO_FLOOR):
        """rgk_render_round_demod_device: render_round_device, which gets the same bits, plus D += sum of L_s / div_s and A += sum of
        div_s per pixel, div_s the floored albedo at the first hit of the sample's own camera ray; DEVICE pointers (ints)."""
        cnt = capi.Counters()
        capi.check(self.lib, self.lib.rgk_render_round_demod_device(self.h, C.byref(camera), C.byref(params), tiles, len(tiles), d_accum_ptr, d_count_ptr,
                                                                    d_demod_ptr, d_div_ptr, albedo_floor, C.byref(cnt)))
        return cnt

    def remodulate_device(self, xres, yres, d_in_rgb, d_div_rgb, d_div_count, d_out_rgb, albedo_floor=capi.DEMOD_ALBEDO_FLOOR):
        """rgk_remodulate_device: out = in * (A / n) with d_div_count, or in * floored albedo with d_div_count None (d_div_rgb then an
        albedo plane); DEVICE pointers (ints), the output none of the inputs."""
        capi.check(self.lib, self.lib.rgk_remodulate_device(self.h, xres, yres, d_in_rgb, d_div_rgb, d_div_count, albedo_floor, d_out_rgb))

    def display_measure_device(self, xres, yres, d_rgb, d_count, params):
        """rgk_display_measure_device: the luminance histogram of a frame and the exposure and white point solved from it, a
        capi.DisplayStats; DEVICE pointers (ints), d_count None for an image that is a mean already, params a capi.DisplayParams (its
        ranges are checked here first: ValueError)."""
        params.check()
        stats = capi.DisplayStats()
        capi.check(self.lib, self.lib.rgk_display_measure_device(self.h, xres, yres, d_rgb, d_count, C.byref(params), C.byref(stats)))
        return stats

    def display_encode_device(self, xres, yres, d_rgb, d_count, params, stats, d_out_rgba):
        """rgk_display_encode_device: params.op with stats.exposure and stats.white -> one R, G, B, 255 word per pixel at d_out_rgba;
        DEVICE pointers (ints), d_count None for an image that is a mean already."""
        params.check()
        capi.check(self.lib, self.lib.rgk_display_encode_device(self.h, xres, yres, d_rgb, d_count, C.byref(params), C.byref(stats), d_out_rgba))

    def write_exr_device(self, path, xres, yres, d_rgb, d_count=None, output_scale=1.0):
        """rgk_output_write_exr_device: the EXR the host writers produce, assembled on the GPU from DEVICE pointers (ints).  d_count:
        accumulator mode (output_scale <= 0: auto); None: d_rgb is an image and output_scale (> 0, finite) multiplies it.  Returns the
        scale applied."""
        val = C.c_float(0.0)
        capi.check(self.lib, self.lib.rgk_output_write_exr_device(self.h, str(path).encode(), xres, yres, d_rgb, d_count, float(output_scale), C.byref(val)))
        return val.value

    def write_png_device(self, path, xres, yres, d_rgba):
        """rgk_output_write_png_device: the PNG rgk_output_write_png produces, from the words of display_encode_device on the device."""
        capi.check(self.lib, self.lib.rgk_output_write_png_device(self.h, str(path).encode(), xres, yres, d_rgba))

    def post_timing(self, which):
        """HIP-event times (ms) of the launches of the last feature pass (0) / denoise call (1) / variance-guided denoise call (2) /
        noise estimate (3) / round fold (4: the copy of its tile list, the fold) / temporal pair (5: reproject, blend) /
        followed feature pass (6: list + ray generation, then walker and k_aov_hop per hop) / upsample call (7: prepare, gather) /
        remodulate call (8) / demodulated round (9: its divisor launches, its second resolves, summed over the passes) /
        display measure (10: the clear of the histogram, k_display_hist) / display encode (11: k_display_encode) /
        device EXR (12: k_out_max or 0, k_out_pack_exr) / device PNG (13: k_out_pack_png, k_out_png_sums);
        set_tuning(time_post=1) first."""
        ms, n = (C.c_double * 32)(), C.c_uint32(32)
        capi.check(self.lib, self.lib.rgk_scene_get_post_timing(self.h, which, ms, C.byref(n)))
        return list(ms[:min(n.value, 32)])

    def render_round_device(self, camera, params, tiles, d_accum_ptr, d_count_ptr):
        cnt = capi.Counters()
        capi.check(self.lib, self.lib.rgk_render_round_device(self.h, C.byref(camera), C.byref(params), tiles, len(tiles),
                                                              d_accum_ptr, d_count_ptr, C.byref(cnt)))
        return cnt


def adapt_select(tiles, visits, xres, yres, params, tile_size=TILE_SIZE):
    """rgk_adapt_select (host only): the tiles the next round still renders.  tiles: the (tiles_y, tiles_x) statistics of
    noise_estimate_device; visits: rounds each tile was rendered in, same order; params: capi.AdaptParams.
    -> (live: (tiles_y, tiles_x) bool, n_live, done)."""
    lib = capi.load_product()
    st = np.ascontiguousarray(tiles, dtype=NOISE_TILE_DTYPE)
    vis = np.ascontiguousarray(visits, dtype=np.uint32)
    ty, tx = tile_grid(xres, yres, tile_size)
    if st.size != ty * tx or vis.size != ty * tx:
        raise ValueError(f"{ty} x {tx} tiles expected, got {st.size} statistics and {vis.size} visit counts")
    live = np.zeros(ty * tx, np.uint8)
    n_live, done = C.c_uint32(0), C.c_uint32(0)
    capi.check(lib, lib.rgk_adapt_select(st.ctypes.data, vis.ctypes.data, xres, yres, tile_size, C.byref(params), live.ctypes.data,
                                         C.byref(n_live), C.byref(done)))
    return live.astype(bool).reshape(ty, tx), n_live.value, bool(done.value)


def sampler_eval(seed, index, dim, is2d):
    lib = capi.load_product()
    seed = np.ascontiguousarray(seed, dtype=np.uint32)
    index = np.ascontiguousarray(index, dtype=np.uint32)
    dim = np.ascontiguousarray(dim, dtype=np.uint32)
    out = np.zeros((len(seed), 2), dtype=np.float32)
    capi.check(lib, lib.rgk_sampler_eval(len(seed), seed.ctypes.data, index.ctypes.data, dim.ctypes.data, int(is2d), out.ctypes.data))
    return out


def read_exr(path):
    """Minimal reader for the files rgk_output_write_exr writes (uncompressed scan-line half RGBA): (h, w, 4) float32
    in R, G, B, A order.  Test infrastructure for the round trip, not a general OpenEXR reader."""
    import struct
    b = open(path, "rb").read()
    assert struct.unpack_from("<ii", b, 0) == (20000630, 2)
    pos, attrs = 8, {}
    while b[pos] != 0:
        e = b.index(b"\0", pos); name = b[pos:e].decode(); pos = e + 1
        e = b.index(b"\0", pos); typ = b[pos:e].decode(); pos = e + 1
        (size,) = struct.unpack_from("<i", b, pos); pos += 4
        attrs[name] = (typ, b[pos:pos + size]); pos += size
    pos += 1
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    assert attrs["compression"][1] == b"\0"
    chans, cp, cl = [], 0, attrs["channels"][1]
    while cl[cp] != 0:
        e = cl.index(b"\0", cp); chans.append(cl[cp:e].decode()); cp = e + 1 + 16
    offs = struct.unpack_from("<%dQ" % h, b, pos)
    img = np.zeros((h, w, 4), np.float32)
    for y in range(h):
        yy, n = struct.unpack_from("<ii", b, offs[y])
        line = np.frombuffer(b, dtype=np.float16, count=w * len(chans), offset=offs[y] + 8).reshape(len(chans), w)
        for k, c in enumerate(chans):
            img[yy - y0, :, "RGBA".index(c)] = line[k]
    return img


def write_exr(path, rgb):
    """rgk_output_write_exr of a (y, x, 3) float32 image."""
    lib = capi.load_product()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    capi.check(lib, lib.rgk_output_write_exr(str(path).encode(), rgb.shape[1], rgb.shape[0], rgb.ctypes.data))


def display_table():
    """rgk_display_table: the 256 float32 thresholds of the sRGB bytes (a copy)."""
    lib = capi.load_product()
    return np.ctypeslib.as_array(lib.rgk_display_table(), shape=(256,)).copy()


def display_solve(hist, n_dark, params):
    """rgk_display_solve (host only): exposure and white point from a histogram of 256 counts -> capi.DisplayStats."""
    lib = capi.load_product()
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.shape != (256,):
        raise ValueError(f"256 bins expected, got {h.shape}")
    stats = capi.DisplayStats()
    capi.check(lib, lib.rgk_display_solve(h.ctypes.data, int(n_dark), C.byref(params), C.byref(stats)))
    return stats


def write_png(path, rgba):
    """rgk_output_write_png of a (y, x, 4) uint8 image (R, G, B, anything; a torch tensor or an array): 8-bit truecolour, the fourth
    byte dropped."""
    lib = capi.load_product()
    if hasattr(rgba, "cpu"):
        rgba = rgba.cpu().numpy()
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError(f"a (y, x, 4) uint8 image expected, got {rgba.shape}")
    capi.check(lib, lib.rgk_output_write_png(str(path).encode(), rgba.shape[1], rgba.shape[0], rgba.ctypes.data))


def on_scene_gpu(scene, *tensors):
    """Whether the device writers can take these tensors: a scene, and every tensor on its GPU."""
    return scene is not None and all(t.is_cuda and t.device.index == scene.device for t in tensors)


def write_exr_image(path, image, val=1.0, scene=None):
    """The EXR of image * val, image a (y, x, 3) float32 torch tensor: through rgk_output_write_exr_device when `scene` is given, the
    tensor lives on its GPU and val is finite and > 0; else write_exr of a host copy.  The same bytes either way."""
    import math
    import torch
    if on_scene_gpu(scene, image) and math.isfinite(val) and val > 0.0:
        image = image.contiguous()
        torch.cuda.current_stream(image.device).synchronize()
        scene.write_exr_device(path, int(image.shape[1]), int(image.shape[0]), image.data_ptr(), None, val)
    else:
        write_exr(path, (image * val).cpu().numpy())


def write_png_image(path, rgba, scene=None):
    """The PNG of a (y, x, 4) uint8 torch tensor: through rgk_output_write_png_device when `scene` is given and the tensor lives on its
    GPU; else write_png of a host copy.  The same bytes either way."""
    import torch
    if on_scene_gpu(scene, rgba) and rgba.dim() == 3 and rgba.shape[2] == 4 and rgba.dtype == torch.uint8:
        rgba = rgba.contiguous()
        torch.cuda.current_stream(rgba.device).synchronize()
        scene.write_png_device(path, int(rgba.shape[1]), int(rgba.shape[0]), rgba.data_ptr())
    else:
        write_png(path, rgba)


def png_beside(path):
    """The PNG that goes with an EXR: the same stem."""
    import os
    return os.path.splitext(str(path))[0] + ".png"


class EXRTexture:
    """The Radiance accumulator (reference src/texture.hpp:83-118); device-resident torch tensors."""

    def __init__(self, xsize, ysize, device):
        import torch
        self.xsize, self.ysize = xsize, ysize
        self.data = torch.zeros((ysize, xsize, 3), dtype=torch.float32, device=device)
        self.count = torch.zeros((ysize, xsize), dtype=torch.int32, device=device)  # bit pattern of uint32

    def get_pixels(self):
        """EXRTexture::GetPixel for every pixel: data / count, 0 where count == 0 (texture.cpp:349-354)."""
        import torch
        c = self.count.to(torch.float32).unsqueeze(-1)
        return torch.where(c > 0, self.data / c.clamp(min=1), torch.zeros_like(self.data))

    def normalize(self, val):
        """EXRTexture::Normalize (texture.cpp:376-400): val <= 0 -> scale so the brightest channel is 1 (Q17)."""
        px = self.get_pixels()
        if val <= 0.0:
            val = 1.0 / float(px.max())
        return px * val

    def write(self, path, output_scale=-1.0, scene=None):
        """total_ob.Normalize(cfg->output_scale).Write(output_file) (render_driver.cpp:233,245) through the C ABI:
        rgk_output_normalize + rgk_output_write_exr on host copies of the accumulator -- or, with `scene` and the accumulator on its
        GPU, rgk_output_write_exr_device where it is: the same bytes.  Returns the scale used."""
        if on_scene_gpu(scene, self.data, self.count):
            import torch
            torch.cuda.current_stream(self.data.device).synchronize()
            return scene.write_exr_device(path, self.xsize, self.ysize, self.data.data_ptr(), self.count.data_ptr(), float(output_scale))
        lib = capi.load_product()
        acc = np.ascontiguousarray(self.data.cpu().numpy(), dtype=np.float32)
        cnt = np.ascontiguousarray(self.count.cpu().numpy()).view(np.uint32)
        out = np.empty_like(acc)
        val = C.c_float(0.0)
        capi.check(lib, lib.rgk_output_normalize(acc.ctypes.data, cnt.ctypes.data, self.xsize, self.ysize, float(output_scale),
                                                 out.ctypes.data, C.byref(val)))
        capi.check(lib, lib.rgk_output_write_exr(str(path).encode(), self.xsize, self.ysize, out.ctypes.data))
        return val.value

    def save(self, path, device_index, tag, rounds_done, seedcount):
        """rgk_accum_save: this accumulator with `tag`, the rounds done and the running task counter."""
        lib = capi.load_product()
        acc = C.c_void_p()
        capi.check(lib, lib.rgk_accum_create(self.xsize, self.ysize, device_index, C.byref(acc)))
        try:
            a = np.ascontiguousarray(self.data.cpu().numpy(), dtype=np.float32)
            c = np.ascontiguousarray(self.count.cpu().numpy()).view(np.uint32)
            capi.check(lib, lib.rgk_accum_upload(acc, a.ctypes.data, c.ctypes.data))
            capi.check(lib, lib.rgk_accum_set_tag(acc, tag))
            capi.check(lib, lib.rgk_accum_save(acc, str(path).encode(), rounds_done, seedcount))
        finally:
            lib.rgk_accum_destroy(acc)

    def load(self, path, device_index, tag):
        """rgk_accum_load, which refuses a file with another tag -> (rounds_done, seedcount) of the saved run."""
        import torch
        lib = capi.load_product()
        acc = C.c_void_p()
        capi.check(lib, lib.rgk_accum_create(self.xsize, self.ysize, device_index, C.byref(acc)))
        try:
            rd_, sc_ = C.c_uint32(0), C.c_uint32(0)
            capi.check(lib, lib.rgk_accum_set_tag(acc, tag))
            capi.check(lib, lib.rgk_accum_load(acc, str(path).encode(), C.byref(rd_), C.byref(sc_)))
            a = np.empty((self.ysize, self.xsize, 3), np.float32)
            c = np.empty((self.ysize, self.xsize), np.uint32)
            capi.check(lib, lib.rgk_accum_download(acc, a.ctypes.data, c.ctypes.data))
        finally:
            lib.rgk_accum_destroy(acc)
        self.data.copy_(torch.from_numpy(a))
        self.count.copy_(torch.from_numpy(c.view(np.int32)))
        return rd_.value, sc_.value


def missing_demod_message(path, suffix):
    return (f"`{path}` has no `{path}{suffix}` beside it: it was written without demodulated accumulation, and the irradiance sums "
            "cannot be continued from it (render without --demod, or start the frame again)")


def missing_half_message(path):
    return (f"`{path}` has no half-buffer `{path}.half` beside it: it was written without noise tracking, and the noise estimate "
            "cannot be continued from it (render without --noise, or start the frame again)")


class TemporalHistory:
    """What one frame of a camera animation hands to the next (static geometry, moving camera): the frame's camera, its depth /
    normal / tri feature planes, and the history image -- demodulated colour (y, x, 3) and length (y, x), float32 tensors on the
    device -- with the capi.TemporalParams both kernels run with.  One object serves a sequence of RenderDrivers, one per frame;
    each commits once (RenderDriver.denoise_temporal).  Lives on the device only: not checkpointed."""

    def __init__(self, params=None):
        self.params = (params or capi.TemporalParams()).check()
        self.reset()

    def reset(self):
        """Forget the chain: the next frame starts with every length 0."""
        self.camera = self.depth = self.normal = self.tri = self.rgb = self.length = None
        self.share = None  # of the last frame's pixels, those that found history (None: that frame started the chain)

    @property
    def empty(self):
        return self.camera is None

    def commit(self, camera, aov, rgb, length):
        self.camera = capi.Camera.from_buffer_copy(camera)
        self.depth, self.normal, self.tri = aov["depth"], aov["normal"], aov["tri"]
        self.rgb, self.length = rgb, length


class RenderDriver:
    """RenderDriver::RenderFrame / RenderRound for one process per GPU."""

    def __init__(self, scene, cfg, camera, rank=0, world_size=1, device=None, sampler=capi.SAMPLER_HALTON, flags=0,
                 host_reduce=False, track_noise=False, adaptive=None, history=None, aov_hops=0, track_demod=False,
                 albedo_floor=capi.DEMOD_ALBEDO_FLOOR, device_output=True):
        import torch
        # device_output: render_frame's EXR and PNG files are assembled on the GPU (rgk_output_write_exr_device /
        # rgk_output_write_png_device) when the tensors live on the scene's GPU; False: on the host from downloaded copies, which CPU
        # tensors get anyway.  The files are byte-identical.
        self.device_output = bool(device_output)
        # track_demod: rounds go through rgk_render_round_demod_device and keep, beside total_ob (which gets the bits it gets without),
        # demod_ob = D, the sum of each sample's radiance over the floored albedo at ITS OWN first hit, and div_ob = A, the sum of those
        # divisors; denoise() and upsample() then filter D / n with demodulate = 0 and multiply back (rgk_remodulate_device).
        # albedo_floor: the floor on a sample's divisor, and on the full-resolution albedo upsample() multiplies back with.
        # Everything that keeps a second accumulator of its own, or more than one rank, is refused, not half-supported.
        self.track_demod = bool(track_demod)
        if self.track_demod:
            clash = [why for on, why in (
                (track_noise, "track_noise: the half-buffers of the irradiance sums that the noise estimate would need are not kept"),
                (adaptive is not None, "adaptive: it needs track_noise"),
                (history is not None, "history: temporal reuse of irradiance is not done"),
                (int(aov_hops) > 0, "aov_hops > 0: the per-sample divisor is the first hit's, not the followed one"),
                (world_size > 1, "world_size > 1: the irradiance sums are not reduced across ranks"),
                (int(cfg.get_params(sampler=sampler, flags=flags).reverse) > 0, "reverse > 0: a light-tracing splat has no sample to demodulate")) if on]
            if clash:
                raise ValueError("track_demod cannot be combined with " + clash[0])
            if not (float(albedo_floor) >= 0.0 and float(albedo_floor) != float("inf")):
                raise ValueError(f"albedo_floor must be >= 0 and finite, got {albedo_floor}")
        self.albedo_floor = float(albedo_floor)
        # aov_hops (0 .. capi.AOV_MAX_HOPS): render_aov() -- and with it denoise(), denoise_variance() and the aov_files -- takes its
        # planes from rgk_render_aov_chain_device, which follows mirrors and glass to the first other surface; aov_hops_plane() is
        # the number of such surfaces a pixel passed.  0: the first-hit planes, every code path the one without it.
        aov_hops = int(aov_hops)
        if not 0 <= aov_hops <= capi.AOV_MAX_HOPS:
            raise ValueError(f"aov_hops must be 0 .. {capi.AOV_MAX_HOPS}")
        if aov_hops > 0 and history is not None:
            raise ValueError("aov_hops > 0 cannot be combined with history=: the reproject step tests the history against first-hit "
                             "geometry, and reprojecting the virtual images behind mirrors and glass is not done")
        self.aov_hops = aov_hops
        # history (a TemporalHistory shared by the drivers of an animation's frames): denoise_temporal() reprojects the previous
        # frame's history into this frame, blends this frame's samples in and commits the result for the next frame.  Nothing else
        # reads it: rounds, accumulator and denoise() are the same with and without one.
        if history is not None and track_noise:
            raise ValueError("temporal reuse cannot be combined with track_noise: the variance-guided filter needs the two halves of "
                             "one frame and stays a per-frame tool")
        self.history = history
        self._reprojected = None  # the history as this frame received it: (rgb, length), made by the first denoise_temporal()
        self.scene, self.cfg, self.camera = scene, cfg, camera
        self.rank, self.world_size = rank, world_size
        self.device = device if device is not None else torch.device("cuda", scene.device)
        self.params = cfg.get_params(sampler=sampler, flags=flags)
        self.tasks = generate_task_list(cfg.xres, cfg.yres, SEEDSTART, 0)
        self.n_tasks = len(self.tasks)
        self.seedcount = 0
        self.total_ob = EXRTexture(cfg.xres, cfg.yres, self.device)
        self.rounds_done = 0
        self.counters = []
        self.host_reduce = host_reduce  # gloo rehearsal: reduce through host copies instead of RCCL
        self.round_ob = None
        self.clock = time.time
        self.checkpoint_tag = 0  # digest of scene + camera + parameters (rgk_accum_set_tag); 0: checkpoints are not compared
        self.aov = None  # the frame's feature planes once render_aov() has made them
        self.display_stats = None  # render_frame(display=...): the capi.DisplayStats of the last rewrite's pictures
        # track_noise: rank 0 keeps a second accumulator, the sum of the ODD rounds (the second, fourth, ...), for the half-buffer
        # noise estimate.  A single-rank driver then renders every round into the per-round accumulator (the one a multi-rank
        # driver has anyway) and one launch over the rendered tiles folds it into total_ob, into half_ob too on odd rounds, and
        # clears it (rgk_round_fold_device): when a round is one pass -- one addition per pixel -- total_ob has the bits it has
        # without tracking (0 + s == s); a round of several passes adds its passes to 0 first instead of to the running total,
        # which may differ in the last place.  Off: every code path is the untracked one.
        self.track_noise = bool(track_noise)
        self.half_ob = EXRTexture(cfg.xres, cfg.yres, self.device) if self.track_noise and rank == 0 else None
        # (their count planes are not kept up: the sample count of all three is total_ob's; a checkpoint copies it in)
        self.demod_ob = EXRTexture(cfg.xres, cfg.yres, self.device) if self.track_demod else None
        self.div_ob = EXRTexture(cfg.xres, cfg.yres, self.device) if self.track_demod else None
        # adaptive (a capi.AdaptParams; its target is render_frame's until_noise): a round renders a subset of the tiles -- those
        # rgk_adapt_select leaves live -- and the fold's odd rounds are each TILE's odd visits.
        # `visits`: rounds each tile was rendered in, in the row-major tile order of noise()["tiles"]; `task_tile`: for task i of
        # the centre-out list, its index there.  None: every code path is the one without it.
        self.adaptive = adaptive
        if adaptive is not None:
            if not self.track_noise:
                raise ValueError("adaptive tile sampling needs track_noise=True: it retires tiles on the half-buffer noise estimate")
            if int(self.params.reverse) > 0:
                raise ValueError("adaptive tile sampling cannot be combined with reverse > 0: light-tracing splats land in tiles that "
                                 "gained no sample count that round, which biases them")
            if world_size > 1:
                raise ValueError("adaptive tile sampling needs world_size == 1: the root adds a constant count per round")
            if int(adaptive.min_visits) < 2:
                raise ValueError("adaptive min_visits must be >= 2: a tile is not estimable before its second visit")
            tx = tile_grid(cfg.xres, cfg.yres)[1]
            self.task_tile = np.array([(t.y0 // TILE_SIZE) * tx + t.x0 // TILE_SIZE for t in self.tasks], dtype=np.int64)
            self.visits = np.zeros(self.n_tasks, dtype=np.uint32)

    def render_round(self, reduce=True, live=None):
        """One RenderRound: every rank renders its tiles into its private accumulator, then ONE sum-reduce of the RGB
        accumulator to rank 0 (no data-path collective inside the round).  Sample counts are not exchanged: every tile
        list covers the frame and every pixel of it gains `multisample` samples per round, splats add none
        (tracer.cpp:18,25), so rank 0 adds that constant itself.
        live (adaptive drivers): a mask over the tiles in the order of noise()["tiles"]; only those are rendered.  None: all.  The
        task counter advances by the whole list either way: a tile carries the seed it has in a uniform frame's round."""
        import torch
        if live is not None and self.adaptive is None:
            raise ValueError("render_round(live=...) needs an adaptive driver")
        tiles = generate_task_list(self.cfg.xres, self.cfg.yres, SEEDSTART, self.seedcount)
        self.seedcount += len(tiles)  # `c = seedcount++` per task, render_driver.cpp:160
        which = self.task_tile if self.adaptive is not None else None  # adaptive: the rendered tiles' indices in `visits`
        if self.world_size > 1:
            tiles = shard_tiles(tiles, self.rank, self.world_size)
        elif live is not None:
            mask = np.asarray(live, dtype=bool).reshape(-1)
            if mask.shape != (self.n_tasks,):
                raise ValueError(f"live: {self.n_tasks} tiles expected, got {mask.size}")
            idx = np.flatnonzero(mask[self.task_tile])  # centre-out order, as the whole list has it
            tiles = (capi.Tile * len(idx))(*[tiles[i] for i in idx])
            which = self.task_tile[idx]
        # The untracked single-rank round accumulates in place.  Every other one renders into the per-round accumulator, which is
        # all zero between rounds: whatever takes a round out of it clears it.
        ob = self.total_ob
        if self.world_size > 1 or self.track_noise:
            if self.round_ob is None:
                self.round_ob = EXRTexture(self.cfg.xres, self.cfg.yres, self.device)
            ob = self.round_ob
        torch.cuda.current_stream(self.device).synchronize()
        if self.track_demod:  # (single rank, untracked: ob is total_ob)
            cnt = self.scene.render_round_demod_device(self.camera, self.params, tiles, ob.data.data_ptr(), ob.count.data_ptr(),
                                                       self.demod_ob.data.data_ptr(), self.div_ob.data.data_ptr(), self.albedo_floor)
        else:
            cnt = self.scene.render_round_device(self.camera, self.params, tiles, ob.data.data_ptr(), ob.count.data_ptr())
        if self.world_size > 1:
            if reduce:
                self._reduce_round()
            ob.data.zero_()
            ob.count.zero_()
        elif self.track_noise:
            to_half = np.full(len(tiles), self.rounds_done & 1, np.uint8) if which is None else self.visits[which] & 1
            self.scene.round_fold_device(self.cfg.xres, self.cfg.yres, tiles, to_half, ob.data.data_ptr(), ob.count.data_ptr(),
                                         self.total_ob.data.data_ptr(), self.total_ob.count.data_ptr(), self.half_ob.data.data_ptr(),
                                         self.half_ob.count.data_ptr())
            if which is not None:
                self.visits[which] += 1
        self.rounds_done += 1
        self.counters.append(cnt)
        return cnt

    def _reduce_round(self):
        """The ranks' per-round accumulators summed to rank 0, which adds the sum to total_ob, and to half_ob on odd rounds."""
        import torch.distributed as dist
        red = self.round_ob.data.cpu() if self.host_reduce else self.round_ob.data
        dist.reduce(red, dst=0, op=dist.ReduceOp.SUM)
        if self.rank == 0:
            red = red.to(self.device)
            for dst in (self.total_ob, self.half_ob) if self.track_noise and self.rounds_done & 1 else (self.total_ob,):
                dst.data += red
                dst.count += int(self.params.multisample)

    def render_aov(self):
        """First-hit feature planes of the whole frame, one ray per pixel through the pixel centre: a dict of torch tensors
        on the device -- "albedo", "normal" (y, x, 3) float32, "depth" (y, x) float32, "tri" (y, x) int32 (-1: miss).
        On a driver with aov_hops > 0: the planes followed through mirrors and glass (rgk_render_aov_chain_device), and "hops".
        Rendered once per driver (one frame, one camera) and kept.  With several ranks the root alone renders them, the
        whole frame (it is one ray per pixel); the other ranks get None."""
        import torch
        if self.rank != 0:
            return None
        if self.aov is None:
            y, x = self.cfg.yres, self.cfg.xres
            a = {"albedo": torch.empty((y, x, 3), dtype=torch.float32, device=self.device),
                 "normal": torch.empty((y, x, 3), dtype=torch.float32, device=self.device),
                 "depth": torch.empty((y, x), dtype=torch.float32, device=self.device),
                 "tri": torch.empty((y, x), dtype=torch.int32, device=self.device)}
            if self.aov_hops > 0:
                a["hops"] = torch.empty((y, x), dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()
            if self.aov_hops > 0:
                self.scene.render_aov_chain_device(self.camera, self.params, self.tasks, self.aov_hops, a["albedo"].data_ptr(), a["normal"].data_ptr(),
                                                   a["depth"].data_ptr(), a["tri"].data_ptr(), a["hops"].data_ptr())
            else:
                self.scene.render_aov_device(self.camera, self.params, self.tasks, a["albedo"].data_ptr(), a["normal"].data_ptr(),
                                             a["depth"].data_ptr(), a["tri"].data_ptr())
            self.aov = a
        return self.aov

    def aov_hops_plane(self):
        """(y, x) uint8 tensor on the device: the mirror / dielectric / transparent surfaces each pixel's feature chain passed
        before the surface render_aov() reports (all 0 on a driver made with aov_hops=0).  Root rank only."""
        import torch
        a = self.render_aov()
        if a is None:
            return None
        return a["hops"] if "hops" in a else torch.zeros((self.cfg.yres, self.cfg.xres), dtype=torch.uint8, device=self.device)

    def _over_count(self, plane):
        """plane / total_ob's sample count per pixel, 0 where the count is 0 (EXRTexture.get_pixels for a plane that shares the count)."""
        import torch
        c = self.total_ob.count.to(torch.float32).unsqueeze(-1)
        return torch.where(c > 0, plane / c.clamp(min=1), torch.zeros_like(plane))

    def irradiance(self):
        """D / n of a track_demod driver: the mean over a pixel's samples of radiance over the sample's own floored first-hit albedo;
        (y, x, 3) float32 tensor on the device, 0 where no sample fell."""
        if not self.track_demod:
            raise ValueError("irradiance() needs a driver made with track_demod=True")
        return self._over_count(self.demod_ob.data)

    def albedo_mean(self):
        """A / n of a track_demod driver: the mean of the samples' divisors, i.e. the floored first-hit albedo anti-aliased over the
        pixel's footprint (1 for a sample that missed); (y, x, 3) float32 tensor on the device, 0 where no sample fell."""
        if not self.track_demod:
            raise ValueError("albedo_mean() needs a driver made with track_demod=True")
        return self._over_count(self.div_ob.data)

    def default_denoise_params(self):
        """The shipped defaults; sigma_color = DENOISE_SIGMA_K x the mean over pixels of the largest channel of the image -- of
        irradiance() on a track_demod driver, whose filter runs on that image, with demodulate = 0."""
        img = self.irradiance() if self.track_demod else self.total_ob.get_pixels()
        level = float(img.max(dim=-1).values.double().mean())
        return capi.DenoiseParams(sigma_color=DENOISE_SIGMA_K * level if level > 0 else 1.0, demodulate=0 if self.track_demod else 1)

    def noise(self, tile_size=TILE_SIZE):
        """The half-buffer noise estimate of the current accumulator (rgk_noise_estimate_device): {"rel": the frame's relative
        noise sqrt(sum of v / sum of |c|^2), an estimate of rel-L2 against the converged image; "tiles": (tiles_y, tiles_x)
        structured array sum_var / sum_sq / n_estimable; "variance": (y, x) float32 tensor, the raw per-pixel v}.
        None before two rounds, without track_noise, and on ranks other than the root."""
        import torch
        if self.rank != 0 or not self.track_noise or self.rounds_done < 2:
            return None
        var = torch.empty((self.cfg.yres, self.cfg.xres), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        tiles = self.scene.noise_estimate_device(self.cfg.xres, self.cfg.yres, tile_size, self.total_ob.data.data_ptr(), self.total_ob.count.data_ptr(),
                                                 self.half_ob.data.data_ptr(), self.half_ob.count.data_ptr(), var.data_ptr())
        sv = sq = 0.0
        for t in tiles.reshape(-1):  # row-major, in double
            sv += float(t["sum_var"])
            sq += float(t["sum_sq"])
        return {"rel": (sv / sq) ** 0.5 if sq > 0 else 0.0, "tiles": tiles, "variance": var}

    def denoise_variance(self, params=None):
        """The variance-guided filter (rgk_denoise_variance_device) of the current accumulator and its half-buffer:
        (image (y, x, 3), variance of the filtered image (y, x)), float32 tensors on the device.  Needs track_noise and two rounds."""
        import torch
        if self.rank != 0:
            return None
        if not self.track_noise or self.rounds_done < 2:
            raise ValueError("the variance-guided filter needs track_noise=True and two rounds")
        a = self.render_aov()
        params = params or capi.DenoiseVarParams()
        out = torch.empty_like(self.total_ob.data)
        var = torch.empty((self.cfg.yres, self.cfg.xres), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        self.scene.denoise_variance_device(self.cfg.xres, self.cfg.yres, self.total_ob.data.data_ptr(), self.total_ob.count.data_ptr(),
                                           self.half_ob.data.data_ptr(), self.half_ob.count.data_ptr(), a["albedo"].data_ptr(), a["normal"].data_ptr(),
                                           a["depth"].data_ptr(), params, out.data_ptr(), var.data_ptr())
        return out, var

    def denoise(self, params=None, variance=False):
        """The current accumulator's image (data / count, not normalised) through the guided a-trous filter
        (rgk_denoise_device): a (y, x, 3) float32 torch tensor on the device.  The accumulator is not changed.  Root rank only.
        On a track_demod driver the filter runs on D / n with demodulate = 0 (whatever `params` says) and the result is multiplied by
        A / n (rgk_remodulate_device): texture detail inside a pixel's footprint never enters the filter.
        variance=True (needs track_noise): the variance-guided filter instead, `params` then a capi.DenoiseVarParams; while fewer
        than two rounds are done there is no estimate yet and the fixed filter with its defaults runs."""
        import torch
        if self.rank != 0:
            return None
        if variance:
            if not self.track_noise:
                raise ValueError("denoise(variance=True) needs track_noise=True")
            if self.rounds_done >= 2:
                return self.denoise_variance(params)[0]
            params = None
        a = self.render_aov()
        params = params or self.default_denoise_params()
        out = torch.empty_like(self.total_ob.data)
        torch.cuda.current_stream(self.device).synchronize()
        if self.track_demod:
            params = capi.DenoiseParams(params.iterations, params.sigma_color, params.sigma_depth, params.normal_power_log2, 0)
            filtered = torch.empty_like(out)
            self.scene.denoise_device(self.cfg.xres, self.cfg.yres, self.demod_ob.data.data_ptr(), self.total_ob.count.data_ptr(),
                                      a["albedo"].data_ptr(), a["normal"].data_ptr(), a["depth"].data_ptr(), params, filtered.data_ptr())
            self.scene.remodulate_device(self.cfg.xres, self.cfg.yres, filtered.data_ptr(), self.div_ob.data.data_ptr(), self.total_ob.count.data_ptr(),
                                         out.data_ptr(), self.albedo_floor)
            return out
        self.scene.denoise_device(self.cfg.xres, self.cfg.yres, self.total_ob.data.data_ptr(), self.total_ob.count.data_ptr(),
                                  a["albedo"].data_ptr(), a["normal"].data_ptr(), a["depth"].data_ptr(), params, out.data_ptr())
        return out

    def denoise_temporal(self, params=None):
        """The current accumulator's image blended into the history the previous frame left (rgk_temporal_reproject_device,
        rgk_temporal_blend_device, parameters: the history's), through the guided a-trous filter with sample counts of 1
        (rgk_denoise_device; params: a capi.DenoiseParams, default the shipped ones with sigma_color from the blended image), and
        the blend committed as the next frame's history: a (y, x, 3) float32 tensor on the device.  The accumulator is not changed.
        On the first frame of a chain every history length is 0 and the blend is the frame itself.  The history is reprojected
        once per driver: a second call -- after more rounds, say -- blends the accumulator into what this frame RECEIVED, never
        into its own earlier blend, and commits again in place of the first.  Root rank only."""
        import torch
        if self.rank != 0:
            return None
        if self.history is None:
            raise ValueError("denoise_temporal needs a driver made with history=TemporalHistory()")
        hist, tp = self.history, self.history.params
        a = self.render_aov()
        y, x = self.cfg.yres, self.cfg.xres
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        if self._reprojected is None:
            rgb, length = torch.zeros((y, x, 3), dtype=torch.float32, device=self.device), torch.zeros((y, x), dtype=torch.float32, device=self.device)
            share = None
            if not hist.empty and tuple(hist.length.shape) == (y, x) and hist.length.device == rgb.device:
                torch.cuda.current_stream(self.device).synchronize()
                self.scene.temporal_reproject_device(x, y, self.camera, hist.camera, a["depth"].data_ptr(), a["normal"].data_ptr(), a["tri"].data_ptr(),
                                                     hist.depth.data_ptr(), hist.normal.data_ptr(), hist.tri.data_ptr(), hist.rgb.data_ptr(),
                                                     hist.length.data_ptr(), tp, rgb.data_ptr(), length.data_ptr())
                share = float((length > 0).double().mean())
            self._reprojected = (rgb, length, share)
        rgb, length, share = self._reprojected
        out_hist, out_len, out = new(y, x, 3), new(y, x), new(y, x, 3)
        torch.cuda.current_stream(self.device).synchronize()
        self.scene.temporal_blend_device(x, y, self.total_ob.data.data_ptr(), self.total_ob.count.data_ptr(), a["albedo"].data_ptr(), rgb.data_ptr(),
                                         length.data_ptr(), tp, out_hist.data_ptr(), out_len.data_ptr(), out.data_ptr())
        if params is None:
            level = float(out.max(dim=-1).values.double().mean())
            params = capi.DenoiseParams(sigma_color=DENOISE_SIGMA_K * level if level > 0 else 1.0)
        ones = torch.ones((y, x), dtype=torch.int32, device=self.device)
        filtered = torch.empty_like(out)
        torch.cuda.current_stream(self.device).synchronize()
        self.scene.denoise_device(x, y, out.data_ptr(), ones.data_ptr(), a["albedo"].data_ptr(), a["normal"].data_ptr(), a["depth"].data_ptr(), params,
                                  filtered.data_ptr())
        hist.commit(self.camera, a, out_hist, out_len)
        hist.share = share
        return filtered

    def default_upsample_params(self):
        """The shipped defaults of the guided upsampler (capi.UpsampleParams)."""
        return capi.UpsampleParams()

    def upsample(self, camera, xres, yres, params=None, denoise=None):
        """The current accumulator -- this driver's grid is the LOW side -- reconstructed on the xres x yres grid of `camera`
        (rgk_upsample_device), guided by this driver's feature planes and those of (camera, xres, yres), which are rendered once and
        kept: (rgb (yres, xres, 3) float32, support (yres, xres) uint8) tensors on the device; not normalised, the accumulator is not
        changed.  support: 1 where the four bilinear taps served, 2 where the 4 x 4 ring did, 0 where the pixel has the nearest low
        pixel's plain colour.  denoise (a capi.DenoiseParams, or True for the shipped ones): rgb then goes through the guided a-trous filter with the full
        grid's planes and sample counts of 1 (rgk_denoise_device), as denoise_temporal's blend does.  Root rank only.
        On a track_demod driver the low accumulator handed over is D, with demodulate = 0 in the upsampler and in the filter (whatever
        the parameters say), and the result is multiplied by the full grid's albedo plane through the floor rule
        (rgk_remodulate_device, albedo_floor the driver's): the full-resolution texture detail comes back without a division of a
        box-averaged radiance by a centre-ray albedo."""
        import torch
        if self.rank != 0:
            return None
        if self.aov_hops > 0:
            raise ValueError("upsample cannot be combined with aov_hops > 0: both grids are tested against first-hit geometry")
        params = (params or self.default_upsample_params()).check()
        if self.track_demod:
            params = capi.UpsampleParams(params.plane_tol, params.normal_cos, 0, params.albedo_floor)
        low = self.render_aov()
        key = (bytes(camera), int(xres), int(yres))
        if getattr(self, "_up_key", None) != key:
            prm = capi.Params.from_buffer_copy(self.params)
            prm.xres, prm.yres = xres, yres
            full = {"albedo": torch.empty((yres, xres, 3), dtype=torch.float32, device=self.device),
                    "normal": torch.empty((yres, xres, 3), dtype=torch.float32, device=self.device),
                    "depth": torch.empty((yres, xres), dtype=torch.float32, device=self.device)}
            torch.cuda.current_stream(self.device).synchronize()
            self.scene.render_aov_device(camera, prm, generate_task_list(xres, yres, SEEDSTART, 0), full["albedo"].data_ptr(), full["normal"].data_ptr(),
                                         full["depth"].data_ptr(), None)
            self._up_key, self._up_aov = key, full
        full = self._up_aov
        out = torch.empty((yres, xres, 3), dtype=torch.float32, device=self.device)
        support = torch.empty((yres, xres), dtype=torch.uint8, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        self.scene.upsample_device(xres, yres, camera, full["albedo"].data_ptr(), full["normal"].data_ptr(), full["depth"].data_ptr(),
                                   self.cfg.xres, self.cfg.yres, self.camera, (self.demod_ob if self.track_demod else self.total_ob).data.data_ptr(), self.total_ob.count.data_ptr(),
                                   low["albedo"].data_ptr(), low["normal"].data_ptr(), low["depth"].data_ptr(), params, out.data_ptr(), support.data_ptr())
        if denoise is True:  # the shipped defaults, sigma_color from the upsampled image as default_denoise_params takes it from the accumulator's
            level = float(out.max(dim=-1).values.double().mean())
            denoise = capi.DenoiseParams(sigma_color=DENOISE_SIGMA_K * level if level > 0 else 1.0)
        if denoise is not None and denoise is not False:
            if self.track_demod:
                denoise = capi.DenoiseParams(denoise.iterations, denoise.sigma_color, denoise.sigma_depth, denoise.normal_power_log2, 0)
            ones = torch.ones((yres, xres), dtype=torch.int32, device=self.device)
            filtered = torch.empty_like(out)
            torch.cuda.current_stream(self.device).synchronize()
            self.scene.denoise_device(xres, yres, out.data_ptr(), ones.data_ptr(), full["albedo"].data_ptr(), full["normal"].data_ptr(), full["depth"].data_ptr(),
                                      denoise, filtered.data_ptr())
            out = filtered
        if self.track_demod:
            remod = torch.empty_like(out)
            torch.cuda.current_stream(self.device).synchronize()
            self.scene.remodulate_device(xres, yres, out.data_ptr(), full["albedo"].data_ptr(), None, remod.data_ptr(), self.albedo_floor)
            out = remod
        return out, support

    def display(self, image=None, params=None, stats=None):
        """A display image: exposure, tone curve and the sRGB transfer function to 8 bits (rgk_display_measure_device,
        rgk_display_encode_device) -> ((y, x, 4) uint8 tensor on the device, bytes R, G, B, 255; the capi.DisplayStats used).
        image None: the current accumulator (data / count, not normalised; not changed).  Else a (y, x, 3) float32 tensor on the
        device that is a mean already -- denoise()'s or upsample()'s result, at any resolution.  params: a capi.DisplayParams,
        default the shipped ones (filmic, automatic exposure).  stats: what an earlier call returned -- its exposure and white are
        used and nothing is measured, so that several images of one frame are comparable.  Root rank only."""
        import torch
        if self.rank != 0:
            return None
        params = (params or capi.DisplayParams()).check()
        if image is None:
            rgb, count = self.total_ob.data, self.total_ob.count
        else:
            if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.float32 or not image.is_cuda:
                raise ValueError("display(image=...) takes a (y, x, 3) float32 tensor on the device")
            rgb, count = image.contiguous(), None
        y, x = int(rgb.shape[0]), int(rgb.shape[1])
        out = torch.empty((y, x, 4), dtype=torch.uint8, device=rgb.device)
        torch.cuda.current_stream(self.device).synchronize()
        d_count = None if count is None else count.data_ptr()
        if stats is None:
            stats = self.scene.display_measure_device(x, y, rgb.data_ptr(), d_count, params)
        self.scene.display_encode_device(x, y, rgb.data_ptr(), d_count, params, stats, out.data_ptr())
        return out, stats

    def save_checkpoint(self, path):
        """Raw-accumulator checkpoint (rgk_accum_save): accumulator + rounds done + the running task counter.  With track_noise the
        half-buffer goes beside it as `<path>.half`, same format, same tag."""
        state = (self.scene.device, self.checkpoint_tag, self.rounds_done, self.seedcount)
        self.total_ob.save(path, *state)
        if self.track_noise:
            self.half_ob.save(str(path) + ".half", *state)
        if self.track_demod:  # `<path>.demod` (D) and `<path>.div` (A): same format, same tag, total_ob's sample counts
            for ob, suffix in ((self.demod_ob, ".demod"), (self.div_ob, ".div")):
                ob.count.copy_(self.total_ob.count)
                ob.save(str(path) + suffix, *state)

    def load_checkpoint(self, path):
        """Resume: the next render_round continues the seed sequence where the saved run stopped.  With track_noise the
        half-buffer `<path>.half` must be there: without it S != S_A + S_B and the estimate would be silently wrong.  With track_demod
        `<path>.demod` and `<path>.div` must be there for the same reason: D and A would cover fewer samples than the count says."""
        import os
        half = str(path) + ".half"
        if self.track_noise and not os.path.exists(half):
            raise RuntimeError(missing_half_message(path))
        if self.track_demod:
            for suffix in (".demod", ".div"):
                if not os.path.exists(str(path) + suffix):
                    raise RuntimeError(missing_demod_message(path, suffix))
        rounds_done, seedcount = self.total_ob.load(path, self.scene.device, self.checkpoint_tag)
        if self.track_demod:
            for ob, suffix in ((self.demod_ob, ".demod"), (self.div_ob, ".div")):
                if ob.load(str(path) + suffix, self.scene.device, self.checkpoint_tag) != (rounds_done, seedcount):
                    raise RuntimeError(f"`{path}{suffix}` was not written together with `{path}`")
        if self.track_noise:
            if self.half_ob.load(half, self.scene.device, self.checkpoint_tag) != (rounds_done, seedcount):
                raise RuntimeError(f"`{half}` was not written together with `{path}`")
        self.rounds_done, self.seedcount = rounds_done, seedcount
        if self.adaptive is not None:
            self.visits = self._visits_from_counts(path)

    def _visits_from_counts(self, path):
        """An adaptive frame's per-tile state needs no file of its own: a tile's visits are its pixels' sample count over
        `multisample`, and the half-buffer holds every second of them.  A tile whose pixels do not all say so is refused."""
        ms = int(self.params.multisample)
        n, nb = (ob.count.cpu().numpy().view(np.uint32) for ob in (self.total_ob, self.half_ob))
        visits = np.zeros(self.n_tasks, dtype=np.uint32)
        for t, k in zip(self.tasks, self.task_tile):
            a, b = n[t.y0:t.y1, t.x0:t.x1], nb[t.y0:t.y1, t.x0:t.x1]
            v = int(a[0, 0]) // ms
            if not ((a == v * ms).all() and (b == (v // 2) * ms).all()):
                raise RuntimeError(f"`{path}`: the tile at ({t.x0}, {t.y0}) is not uniform in its sample counts, or its half-buffer does not "
                                   "hold every second visit: not a frame an adaptive driver can continue")
            visits[k] = v
        return visits

    def adapt_select(self, target, nz=None):
        """rgk_adapt_select on the current noise estimate (nz: what noise() returned, if the caller has it) with this driver's
        visits and min_visits -> (live mask (tiles_y, tiles_x), n_live, done).  Needs two rounds."""
        nz = nz or self.noise()
        if self.adaptive is None or nz is None:
            raise ValueError("adapt_select needs an adaptive driver and two rounds")
        return adapt_select(nz["tiles"], self.visits, self.cfg.xres, self.cfg.yres, capi.AdaptParams(target, self.adaptive.min_visits))

    def _root_decides(self, yes):
        """Rank 0's yes or no, on every rank.  With several ranks a decision to stop or to go on is rank 0's, broadcast to all:
        ranks deciding by their own clocks or estimates could disagree and leave a reduce unmatched."""
        if self.world_size > 1:
            import torch
            import torch.distributed as dist
            flag = torch.tensor([1 if yes else 0], dtype=torch.int32, device="cpu" if self.host_reduce else self.device)
            dist.broadcast(flag, src=0)
            yes = bool(flag.item())
        return yes

    def render_frame(self, rounds=None, minutes=None, output_file=None, checkpoint=None, aov_files=None, denoised_file=None,
                     until_noise=None, noise_file=None, on_noise=None, temporal=False, upsampled_file=None, upsample_to=None,
                     irradiance_file=None, display=None):
        """RenderFrame: Rounds mode (render_driver.cpp:229-235) or Timed mode (:237-247); with `output_file` the
        normalised image is rewritten after every round, as the reference does (rank 0 only).
        aov_files: {"albedo" / "normal" / "depth" / "hops": path} -- the feature planes, written once (depth and hops replicated to
        R, G, B); on a driver with aov_hops > 0 they are the followed planes.
        denoised_file: rewritten after every round that rewrites output_file, normalised with the scale output_file got.
        With track_noise -- until_noise: stop once noise()["rel"] <= until_noise, checked after every round from the second on
        (`rounds` / `minutes` still bound the frame); from the second round on denoised_file comes from the variance-guided
        filter, and noise_file holds sqrt of that filter's output variance in R, G and B, scaled like output_file;
        on_noise(rounds_done, rel) is called on rank 0 after every round that has an estimate.
        With an adaptive driver and until_noise: after every round from the second on rgk_adapt_select (target = until_noise) says
        whether the frame is done and which tiles the next round renders; on_noise(rounds_done, rel, n_live) also gets their number.
        The rule keeps no state, so a frame resumed from a checkpoint goes on with the tiles the interrupted one would have rendered.
        temporal (needs a driver with a history, and denoised_file): after the frame's LAST round denoised_file is rewritten once more,
        from denoise_temporal(), which also commits the history for the next frame; the rewrites after earlier rounds are the
        single-frame filter's as without it.
        upsampled_file with upsample_to = (camera, xres, yres): after every round that rewrites output_file, upsample() to that grid,
        scaled like output_file; filtered with the shipped denoise defaults when there is a denoised_file (which itself stays this
        driver's own resolution).  Not with noise tracking, a history or aov_hops.
        irradiance_file (a track_demod driver): irradiance(), scaled like output_file, after every round that rewrites output_file.
        display (a capi.DisplayParams; needs output_file): every rewrite of output_file, denoised_file and upsampled_file also writes a
        PNG of the same stem beside it (png_beside), made by display() from the image BEFORE its normalisation.  Exposure and white
        point are measured once per rewrite, on the accumulator, and reused for the other two; display_stats keeps the last ones."""
        if display is not None:
            if not output_file:
                raise ValueError("display needs an output_file")
            display.check()
        self.display_stats = None
        out_scene = self.scene if self.device_output else None  # the device writers' scene; None: the host writers

        def picture(path, image=None):
            """The PNG beside `path`: the accumulator's (which measures), or an image's with the accumulator's exposure."""
            if display is not None:
                rgba, st = self.display(image, display, None if image is None else self.display_stats)
                self.display_stats = st
                write_png_image(png_beside(path), rgba, out_scene)
        if irradiance_file and (not self.track_demod or not output_file):
            raise ValueError("irradiance_file needs a driver made with track_demod=True and an output_file")
        if upsampled_file and (upsample_to is None or not output_file or self.track_noise or self.history is not None or self.aov_hops > 0):
            raise ValueError("upsampled_file needs upsample_to=(camera, xres, yres) and an output_file, on a driver without track_noise, history or aov_hops")
        if temporal and (self.history is None or not denoised_file):
            raise ValueError("temporal=True needs a driver made with history=TemporalHistory() and a denoised_file")
        if (until_noise is not None or noise_file or on_noise) and not self.track_noise:
            raise ValueError("until_noise, noise_file and on_noise need track_noise=True")
        rounds = self.cfg.render_rounds if rounds is None else rounds
        minutes = self.cfg.render_minutes if minutes is None else minutes
        t0 = self.clock()
        adapting = self.adaptive is not None and until_noise is not None
        live = None  # the next round's tiles (None: all)
        val = None   # the scale the last rewrite of output_file used
        if aov_files and self.rank == 0:
            a = self.render_aov()
            for name, path in aov_files.items():
                src = self.aov_hops_plane().float() if name == "hops" else a[name]
                plane = src if src.dim() == 3 else src.unsqueeze(-1).expand(-1, -1, 3)
                write_exr_image(path, plane, 1.0, out_scene)
        if adapting and self.rounds_done >= 2:  # resumed
            live, _, done = self.adapt_select(until_noise)
            if done:
                return self.total_ob
        # Rounds mode (render_driver.cpp:229-235), or Timed mode (:237-247): whether another round starts is asked before each
        for _ in range(rounds) if minutes is None else itertools.repeat(None):
            if minutes is not None and not self._root_decides((self.clock() - t0) / 60.0 < minutes):
                break
            self.render_round(live=live)
            if output_file and self.rank == 0:
                val = self.total_ob.write(output_file, getattr(self.cfg, "output_scale", -1.0), out_scene)
                picture(output_file)
                if self.track_noise and self.rounds_done >= 2 and (denoised_file or noise_file):
                    den, var = self.denoise_variance()
                    if denoised_file:
                        write_exr_image(denoised_file, den, val, out_scene)
                        picture(denoised_file, den)
                    if noise_file:
                        write_exr_image(noise_file, var.sqrt().unsqueeze(-1).expand(-1, -1, 3), val, out_scene)
                elif denoised_file:
                    den = self.denoise()
                    write_exr_image(denoised_file, den, val, out_scene)
                    picture(denoised_file, den)
                if irradiance_file:
                    write_exr_image(irradiance_file, self.irradiance(), val, out_scene)
                if upsampled_file:
                    up = self.upsample(*upsample_to, denoise=True if denoised_file else None)[0]
                    write_exr_image(upsampled_file, up, val, out_scene)
                    picture(upsampled_file, up)
            if checkpoint and self.rank == 0:
                self.save_checkpoint(checkpoint)
            nz = self.noise() if on_noise or until_noise is not None else None
            if adapting and nz is not None:
                live, n_live, done = self.adapt_select(until_noise, nz)
                if on_noise:
                    on_noise(self.rounds_done, nz["rel"], n_live)
            else:
                if on_noise and nz is not None:
                    on_noise(self.rounds_done, nz["rel"])
                # (nz is rank 0's: the other ranks have none)
                done = until_noise is not None and self._root_decides(nz is not None and nz["rel"] <= until_noise)
            if done:
                break
        if temporal and val is not None and self.rank == 0:
            den = self.denoise_temporal()
            write_exr_image(denoised_file, den, val, out_scene)
            picture(denoised_file, den)
        return self.total_ob
