"""Padding of a SceneBuilder, for test_pad_cpu.py / test_gpu_thresholds.py: the same scene under other material and texture
numbers and other byte-table offsets, applied before to_desc().

The shading kernels pick a load path by two numbers (rgk_amd/csrc/rgk_device.h): material ids below RGK_LDS_MATERIALS (64) are
read from the copy in LDS, the others from global memory (mat_load); a byte texel is decoded through LDS while its table ends
inside the first RGK_LDS_LUT_FLOATS (512) floats of the table pool, else by three global loads (texel_at / texels_at).  Nothing a
round, a BxDF, a texture lookup or a feature plane computes depends on a material's or a texture's NUMBER, so a scene whose
records have been moved past either threshold must give the bits it gave before.

pad_materials(sb, P)  P filler materials in front of the scene's own; triangle materials, mix children and the name map are
                      renumbered.  The fillers are on no triangle and are no mix child; each is loud (a read of the wrong
                      record changes the result) and none equals a material of the scene: an emissive diffuse, a mirror, a
                      dielectric and an LTC material in turn, with their own colours, index of refraction and roughness.
pad_tables(sb, K)     K 1 x 1 RGK_TEX_RGB8 textures in front of the scene's textures, filler k with its own 256-float table: a
                      seeded permutation of the gamma table times (k + 2).  Texture ids are renumbered.  Caller-supplied tables
                      are laid out in the order of their first appearance (rgk_commit.cpp assign_palettes), so the scene's own
                      byte textures get the table offset 256 K, and the tables of palettized float textures follow.
"""
import numpy as np

from rgk_amd import capi
from rgk_amd.scene import gamma_lut

LDS_MATERIALS = 64       # RGK_LDS_MATERIALS
LDS_LUT_FLOATS = 512     # RGK_LDS_LUT_FLOATS


def filler_material(sb, i):
    """Filler i: its kind by i % 4, every parameter a function of i (no two fillers alike, none like a test scene's material)."""
    c = lambda a, b, d: (0.05 + ((a * i + 1) % 17) / 20.0, 0.05 + ((b * i + 2) % 19) / 22.0, 0.05 + ((d * i + 3) % 23) / 26.0)
    which = i % 4
    if which == 0:
        m = sb.new_material(f"pad{i}", capi.BXDF_DIFFUSE)
        m["tex_diffuse"] = sb.create_solid_texture(c(3, 5, 7))
        m["emission"] = (500.0 + 3.0 * i, 400.0 + 5.0 * i, 300.0 + 7.0 * i)
    elif which == 1:
        m = sb.new_material(f"pad{i}", capi.BXDF_MIRROR)
        m["tex_color"] = sb.create_solid_texture(c(5, 7, 3))
    elif which == 2:
        m = sb.new_material(f"pad{i}", capi.BXDF_DIELECTRIC)
        m["tex_color"] = sb.create_solid_texture(c(7, 3, 5))
        m["ior"] = 1.9 + 0.003 * i
    else:
        m = sb.new_material(f"pad{i}", capi.BXDF_LTC_GGX_DIFFUSE if i % 8 == 3 else capi.BXDF_LTC_BECKMANN)
        m["tex_color"] = sb.create_solid_texture(c(3, 7, 5))
        if m["kind"] == capi.BXDF_LTC_GGX_DIFFUSE:
            m["tex_diffuse"] = sb.create_solid_texture(c(7, 5, 3))
        m["roughness"] = 0.041 + 0.0037 * i
    return m


def pad_materials(sb, P):
    """P fillers in front; returns sb.  (Their solid textures go to the END of the texture list: no texture id moves.)"""
    if P == 0:
        return sb
    assert not any(m["name"].startswith("pad") for m in sb.materials)
    fillers = [filler_material(sb, i) for i in range(P)]
    for m in sb.materials:
        for k in ("mix_m1", "mix_m2"):
            if m[k] >= 0:
                m[k] += P
    sb.materials = fillers + sb.materials
    sb.mat_by_name = {name: i + P for name, i in sb.mat_by_name.items()}
    for i, m in enumerate(fillers):
        sb.mat_by_name[m["name"]] = i
    sb.tri_mat = [(a + np.uint32(P)).astype(np.uint32) for a in sb.tri_mat]
    return sb


def filler_table(k):
    """Table k: a seeded random permutation of the gamma table, times (k + 2) -- 256 floats no other table holds in this order."""
    return (gamma_lut()[np.random.default_rng(9000 + k).permutation(256)] * np.float32(k + 2)).astype(np.float32)


def pad_tables(sb, K):
    """K 1 x 1 byte textures with tables of their own in front; returns sb."""
    if K == 0:
        return sb
    assert not any(str(key).startswith("padtable") for key in sb.tex_by_path)
    fillers = [dict(kind=capi.TEX_RGB8, color=(0.0, 0.0, 0.0), lut=filler_table(k),
                    data=np.random.default_rng(9500 + k).integers(0, 256, (1, 1, 3), dtype=np.uint8)) for k in range(K)]
    sb.textures = fillers + sb.textures
    sb.tex_by_path = {key: i + K for key, i in sb.tex_by_path.items()}
    for k in range(K):
        sb.tex_by_path[f"padtable{k}"] = k
    for m in sb.materials:
        for key in ("tex_diffuse", "tex_color", "tex_bump"):
            if m[key] >= 0:
                m[key] += K
    if sb.sky["tex"] >= 0:
        sb.sky["tex"] += K
    return sb


def pad(sb, P, K):
    return pad_tables(pad_materials(sb, P), K)


def desc_tables(desc):
    """The distinct caller-supplied byte tables of a descriptor in the order of their first appearance (bytes of 256 floats)."""
    seen = []
    for i in range(desc.n_textures):
        t = desc.textures[i]
        if t.kind == capi.TEX_RGB8:
            b = bytes(np.ctypeslib.as_array(t.lut, shape=(256,)).astype(np.float32).tobytes())
            if b not in seen:
                seen.append(b)
    return seen
