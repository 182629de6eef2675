"""CPU expectation for the feature planes that follow mirrors and glass (include/rgk.h rgk_render_aov_chain[_device]), for
test_aov_chain_cpu.py / test_gpu_aov_chain.py, and the "hall" scene both use.

The definition, composed from the oracle library's primitives and sharing no code with the kernel (k_aov_hop, rgk_post.hip):
orc_camera_ray makes ray_0, OracleScene.trace_closest_exhaustive answers every ray -- the tree-free search under the walkers'
stated rule, exact ties included, so no pixel is left out of any comparison -- orc_bxdf_sample at u = U samples the delta
materials, orc_texture_sample reads the textures; the vertex (surface_point()), the quaternion frame, the leak rule and the
next ray are restated here in numpy float32, the same operations in the same order (contraction is off on both sides).

Per pixel, float32.  U = (0x1.fffffep-1f, 0), T_0 = (1, 1, 1), L_0 = 0; ray_0: the centre ray of the pinhole copy of the camera,
near 0, far 10000, no ignored triangle.  For hop k = 0, 1, ...:
  1. trace ray_k.  Miss: tri = -1, depth = 0, normal = albedo = 0, hops = k.  End.
  2. v = the vertex at the hit, L_{k+1} = L_k + t_k.  !v.ok: tri = tri_k, depth = L_{k+1}, normal = albedo = 0, hops = k.  End.
  3. TERMINAL: tri = tri_k, depth = L_{k+1}, normal = v.lightN, albedo = T_k * albedo_of(v.mat, v.uv), hops = k.  End.
     Terminal when the top-level material kind is not mirror / dielectric / transparent, and when k == max_hops.
  4. else (dirL, weight, may_leak) = the BxDF sample at u = U; dir = qrot(qinverse(v.g2l), dirL); the leak rule
     !(dot(dir, faceN) * dot(Vr, faceN) > 0) && !may_leak makes the vertex terminal.
  5. T_{k+1} = T_k * weight; ray_{k+1}: origin v.pos + v.faceN * epsilon * 10 * (dirL.z < 0 ? -1 : 1), direction
     norm3(norm3(dir)), ignored triangle tri_k, near 0, far 10000.  (A ray with a NaN component finds nothing: a miss at k + 1.)

`chain(...)` walks every pixel to RGK_AOV_MAX_HOPS once and keeps, per hop, what the pixel would report if the chain had to end
there; `planes(ch, max_hops)` reads the planes of any max_hops out of it.
"""
import ctypes as C
import functools
import math
import os

import numpy as np

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder

F = np.float32
MAX_HOPS = 8
U = (float.fromhex("0x1.fffffep-1"), 0.0)
DELTA = (capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC, capi.BXDF_TRANSPARENT)
# how a pixel's chain ends / what happened at one of its hops
MISS, DROPPED, SURFACE, LEAK, CONTINUES = 0, 1, 2, 3, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ float32 vector pieces (rgk_device.h's, restated)
def v3(x, y, z):
    return np.array([x, y, z], F)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(x, y):
    return v3(x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1])


def len3(v):
    return np.sqrt(dot3(v, v))


def norm3(v):
    return v * (F(1) / np.sqrt(dot3(v, v)))


def qrot(q, v):  # q = (w, x, y, z); q * v, glm semantics
    qv = v3(q[1], q[2], q[3])
    uv = cross3(qv, v)
    uuv = cross3(qv, uv)
    return v + ((uv * q[0]) + uuv) * F(2)


def qinverse(q):
    d = ((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]) + q[0] * q[0]
    return np.array([q[0] / d, -q[1] / d, -q[2] / d, -q[3] / d], F)


def _libm(L, fn, x):
    a, out = np.array([x], F), np.zeros(1, F)
    L.orc_libm(fn, 1, a.ctypes.data, a.ctypes.data, out.ctypes.data)
    return out[0]


def rotation_between(L, start, dest):
    """RotationBetweenVectors as the integrator has it; (w, x, y, z)."""
    start, dest = norm3(start), norm3(dest)
    cos_theta = dot3(start, dest)
    if cos_theta < F(-1) + F(0.001):
        axis = cross3(v3(0, 1, 0), start)
        if float(len3(axis)) < 0.01:
            axis = cross3(v3(1, 0, 0), start)
        axis = norm3(axis)
        half = F(math.pi) * F(0.5)
        s, c = _libm(L, 0, half), _libm(L, 1, half)
        return np.array([c, axis[0] * s, axis[1] * s, axis[2] * s], F)
    axis = cross3(start, dest)
    s = np.sqrt((F(1) + cos_theta) * F(2))
    invs = F(1) / s
    return np.array([s * F(0.5), axis[0] * invs, axis[1] * invs, axis[2] * invs], F)


# ------------------------------------------------------------------ the scene's tables and the vertex
def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dtype)), shape=(n,)).copy() if n else np.zeros(0)


class Tables:
    def __init__(self, O, osc, desc):
        self.L, self.osc = O.lib(), osc
        nv, nt = desc.n_vertices, desc.n_triangles
        self.normals = _arr(desc.normals, 3 * nv, C.c_float).reshape(-1, 3).astype(F)
        self.tangents = _arr(desc.tangents, 3 * nv, C.c_float).reshape(-1, 3).astype(F)
        self.texc = _arr(desc.texcoords, 2 * nv, C.c_float).reshape(-1, 2).astype(F) if desc.texcoords else None
        self.idx = _arr(desc.tri_indices, 3 * nt, C.c_uint32).reshape(-1, 3)
        self.tmat = _arr(desc.tri_material, nt, C.c_uint32)
        self.mats = [desc.materials[i] for i in range(desc.n_materials)]
        self.eps = F(osc.info().epsilon)

    def tex(self, ti, uv, slopes=False):
        rgb, r, b = (C.c_float * 3)(), C.c_float(), C.c_float()
        self.L.orc_texture_sample(self.osc.h, int(ti), (C.c_float * 2)(float(uv[0]), float(uv[1])), rgb, C.byref(r), C.byref(b))
        return (F(r.value), F(b.value)) if slopes else np.array(rgb[:], F)

    def albedo_leaf(self, m, uv):
        k = m.kind
        if k == capi.BXDF_DIFFUSE:
            return self.tex(m.tex_diffuse, uv)
        if k in (capi.BXDF_LTC_BECKMANN, capi.BXDF_LTC_GGX):
            return self.tex(m.tex_color, uv)
        if k in (capi.BXDF_LTC_BECKMANN_DIFFUSE, capi.BXDF_LTC_GGX_DIFFUSE):
            return self.tex(m.tex_diffuse, uv) + self.tex(m.tex_color, uv)
        if k in DELTA:
            return np.ones(3, F)
        return np.zeros(3, F)

    def albedo_of(self, m, uv, level=0):
        if m.kind != capi.BXDF_MIX:
            return self.albedo_leaf(m, uv)
        if level == 2:
            return np.zeros(3, F)
        a = F(m.amount)
        return a * self.albedo_of(self.mats[m.mix_m1], uv, level + 1) + (F(1) - a) * self.albedo_of(self.mats[m.mix_m2], uv, level + 1)

    def sample_delta(self, mat_id, VrL, uv):
        d, w, leak = (C.c_float * 3)(), (C.c_float * 3)(), C.c_int(0)
        self.L.orc_bxdf_sample(self.osc.h, int(mat_id), (C.c_float * 3)(*[float(x) for x in VrL]), (C.c_float * 2)(float(uv[0]), float(uv[1])),
                               (C.c_float * 2)(*U), d, w, C.byref(leak))
        return np.array(d[:], F), np.array(w[:], F), bool(leak.value)


class Vertex:
    pass


def surface_point(tb, bumpmap_scale, o, d, t, al, be, tri):
    """surface_point() (rgk_device.h): the geometric half of a path vertex."""
    v = Vertex()
    v.mat_id = int(tb.tmat[tri])
    v.mat = tb.mats[v.mat_id]
    ia, ib, ic = F(1) - al - be, al, be
    va, vb, vc = tb.idx[tri]
    v.Vr = -d
    v.pos = o + t * d
    nA, nB, nC = tb.normals[va], tb.normals[vb], tb.normals[vc]
    faceN = ia * nA + ib * nB + ic * nC
    v.ok = True
    if np.isnan(faceN[0]):
        faceN = nA
        if np.isnan(faceN[0]):
            faceN = nB
            if np.isnan(faceN[0]):
                faceN = nC
                if np.isnan(faceN[0]):
                    v.ok = False
    if v.ok and len3(faceN) <= 0:
        v.ok = False
    v.uv = np.zeros(2, F)
    if not v.ok:
        return v
    faceN = norm3(faceN)
    if tb.texc is not None:
        v.uv = (ia * tb.texc[va] + ib * tb.texc[vb] + ic * tb.texc[vc]).astype(F)
    lightN = faceN
    if v.mat.tex_bump >= 0:
        right, bottom = tb.tex(v.mat.tex_bump, v.uv, slopes=True)
        tangent = ia * tb.tangents[va] + ib * tb.tangents[vb] + ic * tb.tangents[vc]
        if not ((tangent[0] * tangent[0] + tangent[1] * tangent[1]) + tangent[2] * tangent[2] < F(0.001)):
            tangent = norm3(tangent)
            bitangent = norm3(cross3(faceN, tangent))
            tangent2 = cross3(bitangent, faceN)
            lightN = norm3(faceN + (tangent2 * right + bitangent * bottom) * F(bumpmap_scale))
            if np.isnan(lightN[0]):
                lightN = faceN
    v.faceN, v.lightN = faceN, lightN
    v.g2l = rotation_between(tb.L, lightN, v3(0, 0, 1))
    v.VrL = qrot(v.g2l, v.Vr)
    return v


# ------------------------------------------------------------------ the chain
def pinhole(camera):
    cam = capi.Camera.from_buffer_copy(camera)
    cam.lens_size = 0.0
    return cam


class Chain:
    """Per hop k (arrays over the frame's pixels, row-major): event[k] (MISS / DROPPED / SURFACE / LEAK / CONTINUES; -1: the chain
    ended before k), and what the pixel reports if its chain ends at k: tri[k], depth[k], normal[k], albedo[k].  reflected[k]: the
    sample at k was a dielectric's reflection (total internal reflection); kind[k]: the material kind met at k; ray[k]: ray_k
    {origin, direction}."""


def chain(O, osc, desc, camera, xres, yres, bumpmap_scale, hops=MAX_HOPS):
    L = O.lib()
    tb = Tables(O, osc, desc)
    cam = pinhole(camera)
    Pn = xres * yres
    sub, lens, out6 = (C.c_float * 2)(0.5, 0.5), (C.c_float * 2)(0.0, 0.0), (C.c_float * 6)()
    rays = np.zeros((Pn, 8), F)
    for p in range(Pn):
        L.orc_camera_ray(C.byref(cam), p % xres, p // xres, xres, yres, sub, lens, out6)
        rays[p, :6] = out6[:]
    rays[:, 6], rays[:, 7] = 0.0, 10000.0
    ch = Chain()
    ch.xres, ch.yres = xres, yres
    ch.event = np.full((hops + 1, Pn), -1, np.int8)
    ch.tri = np.full((hops + 1, Pn), -1, np.int32)
    ch.depth = np.zeros((hops + 1, Pn), F)
    ch.normal = np.zeros((hops + 1, Pn, 3), F)
    ch.albedo = np.zeros((hops + 1, Pn, 3), F)
    ch.reflected = np.zeros((hops + 1, Pn), bool)
    ch.kind = np.full((hops + 1, Pn), -1, np.int8)
    ch.ray = np.zeros((hops + 1, Pn, 6), F)
    live = np.arange(Pn)
    ignore = np.full(Pn, -1, np.int32)
    T = np.ones((Pn, 3), F)
    Lsum = np.zeros(Pn, F)
    old = np.seterr(all="ignore")
    try:
        for k in range(hops + 1):
            if not len(live):
                break
            hits = osc.trace_closest_exhaustive(rays[live], ignore[live])
            ch.ray[k, live] = rays[live, :6]
            nxt = []
            for j, p in enumerate(live):
                tri = int(hits["tri"][j])
                if tri < 0:
                    ch.event[k, p] = MISS
                    continue
                t = F(hits["t"][j])
                o, d = rays[p, 0:3].copy(), rays[p, 3:6].copy()
                v = surface_point(tb, bumpmap_scale, o, d, t, F(hits["b"][j]), F(hits["c"][j]), tri)
                Lk = Lsum[p] + t
                ch.tri[k, p], ch.depth[k, p] = tri, Lk
                if not v.ok:
                    ch.event[k, p] = DROPPED
                    continue
                ch.kind[k, p] = v.mat.kind
                ch.normal[k, p] = v.lightN
                ch.albedo[k, p] = T[p] * tb.albedo_of(v.mat, v.uv)
                if v.mat.kind not in DELTA:
                    ch.event[k, p] = SURFACE
                    continue
                dirL, weight, may_leak = tb.sample_delta(v.mat_id, v.VrL, v.uv)
                dr = qrot(qinverse(v.g2l), dirL)
                if not (dot3(dr, v.faceN) * dot3(v.Vr, v.faceN) > 0) and not may_leak:
                    ch.event[k, p] = LEAK
                    continue
                ch.event[k, p] = CONTINUES
                ch.reflected[k, p] = v.mat.kind == capi.BXDF_DIELECTRIC and not may_leak
                T[p] = T[p] * weight
                Lsum[p] = Lk
                rays[p, 0:3] = v.pos + v.faceN * tb.eps * F(10) * (F(-1) if dirL[2] < 0 else F(1))
                rays[p, 3:6] = norm3(norm3(dr))
                ignore[p] = tri
                nxt.append(p)
            live = np.array(nxt, dtype=np.int64)
    finally:
        np.seterr(**old)
    return ch


def planes(ch, max_hops):
    """(albedo (y, x, 3), normal (y, x, 3), depth (y, x), tri (y, x) int32, hops (y, x) uint8, end (y, x) int8) for max_hops:
    a pixel ends at the first hop whose event is not CONTINUES, or at max_hops as a terminal vertex (end = CONTINUES there)."""
    assert 0 <= max_hops < len(ch.event)
    Pn = ch.event.shape[1]
    ev = ch.event[:max_hops + 1]
    ended = ev != CONTINUES
    e = np.where(ended.any(axis=0), ended.argmax(axis=0), max_hops)
    ar = np.arange(Pn)
    end = ev[e, ar]
    assert (end >= 0).all()
    gone = (end == MISS)
    flat = (end == MISS) | (end == DROPPED)
    tri = np.where(gone, -1, ch.tri[e, ar]).astype(np.int32)
    depth = np.where(gone, F(0), ch.depth[e, ar]).astype(F)
    normal = np.where(flat[:, None], F(0), ch.normal[e, ar]).astype(F)
    albedo = np.where(flat[:, None], F(0), ch.albedo[e, ar]).astype(F)
    y, x = ch.yres, ch.xres
    return (albedo.reshape(y, x, 3), normal.reshape(y, x, 3), depth.reshape(y, x), tri.reshape(y, x), e.astype(np.uint8).reshape(y, x),
            end.reshape(y, x))


# ------------------------------------------------------------------ the hall
HALL_W, HALL_H, HALL_BUMP = 64, 48, 2.0
MIRROR_COLOR = (0.9, 0.7, 0.5)
CHECKER = ((0.8, 0.8, 0.75), (0.15, 0.2, 0.3))
PAINT = (0.7, 0.2, 0.2)
SLAB_THICKNESS = 0.1


def _quad(sb, mat, p0, p1, p2, p3, uv=((0, 0), (1, 0), (1, 1), (0, 1)), normal=None):
    """Two triangles p0 p1 p2, p0 p2 p3 with one flat normal (p1 - p0) x (p3 - p0), the tangent along p0 -> p1."""
    p = np.array([p0, p1, p2, p3], np.float64)
    n = np.cross(p[1] - p[0], p[3] - p[0])
    n = n / np.linalg.norm(n) if normal is None else np.array(normal, np.float64)
    t = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    sb.add_mesh(p.astype(F), np.tile(n, (4, 1)).astype(F), np.array(uv, F), np.tile(t, (4, 1)).astype(F), [[0, 1, 2], [0, 2, 3]], sb.material_index(mat))


def _tri(sb, mat, p0, p1, p2):
    p = np.array([p0, p1, p2], np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    n = n / np.linalg.norm(n)
    t = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    sb.add_mesh(p.astype(F), np.tile(n, (3, 1)).astype(F), np.array([(0, 0), (1, 0), (0, 1)], F), np.tile(t, (3, 1)).astype(F), [[0, 1, 2]], sb.material_index(mat))


def _box(sb, mat, lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    _quad(sb, mat, (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))  # +z
    _quad(sb, mat, (x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0))  # -z
    _quad(sb, mat, (x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1))  # +x
    _quad(sb, mat, (x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0))  # -x
    _quad(sb, mat, (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0))  # +y
    _quad(sb, mat, (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))  # -y


def hall():
    """A few hundred triangles under an open sky: a checkered floor; a flat coloured mirror; a glass slab and a glass prism (total
    internal reflection on its slanted face); a bump-mapped mirror lying almost flat (grazing reflections about the tilted normal
    dip under the surface: the leak rule); a transparent quad; a mirror / diffuse mix; a quad without normals (a dropped vertex),
    seen directly and through the transparent quad."""
    sb = SceneBuilder()

    def mat(name, kind, **kw):
        m = sb.new_material(name, kind)
        for k, v in kw.items():
            m[k] = sb.create_solid_texture(v) if k.startswith("tex_") and not isinstance(v, int) else v
        return sb.register_material(m)
    ck = np.zeros((64, 64, 3), F)  # 8 x 8 fields of 8 x 8 texels: inside a field the four texels of a footprint are one colour
    for i in range(64):
        for j in range(64):
            ck[i, j] = CHECKER[((i >> 3) + (j >> 3)) & 1]
    rng = np.random.default_rng(11)
    bump = np.repeat(rng.random((16, 16, 1)).astype(F), 3, axis=2)
    mat("floor", capi.BXDF_DIFFUSE, tex_diffuse=sb.add_image_texture("checker", ck))
    mat("mirror", capi.BXDF_MIRROR, tex_color=MIRROR_COLOR)
    mat("glass", capi.BXDF_DIELECTRIC, tex_color=(1.0, 1.0, 1.0), ior=1.5)
    mat("ghost", capi.BXDF_TRANSPARENT)
    mat("bumpy", capi.BXDF_MIRROR, tex_color=(0.8, 0.8, 0.9), tex_bump=sb.add_image_texture("bump", bump))
    mat("paint", capi.BXDF_DIFFUSE, tex_diffuse=PAINT)
    mat("half", capi.BXDF_MIX, mix_m1=sb.material_index("mirror"), mix_m2=sb.material_index("paint"), amount=0.5)
    mat("dead", capi.BXDF_DIFFUSE, tex_diffuse=(0.5, 0.5, 0.5))
    sb.parts = {}  # name -> range of triangle ids

    def part(name, build):
        first = sb.n_tris
        build()
        sb.parts[name] = range(first, sb.n_tris)

    def floor():  # 10 x 10 cells over [-5, 5]^2, the checker repeated twice each way
        for i in range(10):
            for j in range(10):
                x0, x1, z0, z1 = -5 + i, -4 + i, -5 + j, -4 + j
                uv = [((x + 5) / 5.0, (z + 5) / 5.0) for x, z in ((x0, z1), (x1, z1), (x1, z0), (x0, z0))]
                _quad(sb, "floor", (x0, 0, z1), (x1, 0, z1), (x1, 0, z0), (x0, 0, z0), uv=uv)

    def prism():  # (x, z) of its section: the front faces +z, the face C -> A is the one rays from the front meet beyond the critical angle
        A, B, Cc, y0, y1 = (2.0, 1.0), (3.6, 1.0), (2.8, 0.2), 0.0, 1.2
        _quad(sb, "glass", (A[0], y0, A[1]), (B[0], y0, B[1]), (B[0], y1, B[1]), (A[0], y1, A[1]))
        _quad(sb, "glass", (B[0], y0, B[1]), (Cc[0], y0, Cc[1]), (Cc[0], y1, Cc[1]), (B[0], y1, B[1]))
        _quad(sb, "glass", (Cc[0], y0, Cc[1]), (A[0], y0, A[1]), (A[0], y1, A[1]), (Cc[0], y1, Cc[1]))
        _tri(sb, "glass", (A[0], y1, A[1]), (B[0], y1, B[1]), (Cc[0], y1, Cc[1]))
        _tri(sb, "glass", (A[0], y0, A[1]), (Cc[0], y0, Cc[1]), (B[0], y0, B[1]))
    part("floor", floor)
    part("mirror", lambda: _quad(sb, "mirror", (-4.0, 0.0, -3.0), (-1.0, 0.0, -3.0), (-1.0, 3.0, -3.0), (-4.0, 3.0, -3.0)))  # flat, facing +z
    part("slab", lambda: _box(sb, "glass", (0.2, 0.0, 2.4), (1.6, 1.3, 2.4 + SLAB_THICKNESS)))  # its first two triangles: the +z face
    part("prism", prism)
    part("bumpy", lambda: _quad(sb, "bumpy", (-0.8, 0.05, 1.5), (1.0, 0.05, 1.5), (1.0, 0.25, -1.0), (-0.8, 0.25, -1.0), uv=((0, 0), (2, 0), (2, 3), (0, 3))))
    part("ghost", lambda: _quad(sb, "ghost", (-3.2, 0.1, 3.0), (-1.6, 0.1, 3.0), (-1.6, 1.6, 3.0), (-3.2, 1.6, 3.0)))
    part("half", lambda: _quad(sb, "half", (1.5, 0.0, -2.5), (4.0, 0.0, -2.0), (4.0, 2.5, -2.0), (1.5, 2.5, -2.5)))
    part("dead-behind-ghost", lambda: _quad(sb, "dead", (-2.9, 0.3, 1.0), (-2.3, 0.3, 1.0), (-2.3, 0.9, 1.0), (-2.9, 0.9, 1.0), normal=(0, 0, 0)))
    part("dead", lambda: _quad(sb, "dead", (-0.6, 1.4, 0.0), (-0.1, 1.4, 0.0), (-0.1, 1.9, 0.0), (-0.6, 1.9, 0.0), normal=(0, 0, 0)))
    sb.add_point_light((0.0, 4.5, 3.0), (1.0, 1.0, 1.0), 30.0, 0.0)
    sb.set_skybox_color((0.4, 0.5, 0.7), 1.0)
    return sb


def hall_camera(W=HALL_W, H=HALL_H):
    return make_camera((0.0, 2.8, 6.5), (0.0, 0.3, -0.5), (0, 1, 0), fov=52, xres=W, yres=H)


def hall_params(spp=1, depth=6, W=HALL_W, H=HALL_H):
    return make_params(W, H, spp, depth, bumpscale=HALL_BUMP)


def spheres_case(scale=0.055):
    """The committed Cornell box with an LTC and a dielectric sphere: (builder, camera, xres, yres, bumpmap scale, fixture)."""
    from rgk_amd.workloads import SceneFixture
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_cornell-box-spheres.npz"), scale=scale, spp=4)
    return wl.builder, wl.camera, wl.xres, wl.yres, wl.bumpscale, wl


@functools.lru_cache(maxsize=None)
def reference(name):
    """The chain of a named case, computed once per process: (Chain, desc, builder).  "hall", "spheres"."""
    from oracle import rgk_oracle as O
    if name == "hall":
        sb, cam, W, H, bump = hall(), hall_camera(), HALL_W, HALL_H, HALL_BUMP
    else:
        sb, cam, W, H, bump, _ = spheres_case()
    desc = sb.to_desc()
    osc = O.OracleScene(desc)
    return chain(O, osc, desc, cam, W, H, bump), desc, sb
