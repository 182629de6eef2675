"""numpy restatement of the display stage (include/rgk.h "display output"; rgk_amd/csrc/rgk_display.h): the input colour, the
luminance histogram, the solve, the three curves and the sRGB byte, every float32 operation in the order the definition writes it.
numpy rounds every ufunc result to float32 and fuses nothing, so the words equal the kernels' bit for bit.

The transfer table is an ARGUMENT of encode(): the definition says the table is the transfer function, so the restatement compares
against the library's (rgk_display_table); table() is the double formula the library's must equal to within one float32 ulp."""
import numpy as np

F = np.float32
LINEAR, REINHARD, FILMIC = 0, 1, 2
OPS = {"linear": LINEAR, "reinhard": REINHARD, "filmic": FILMIC}
BINS = 256
BIAS = (127 - 20) << 3
MAX = F(65504.0)


def table():
    """T[0] = 0, T[k] = srgb_to_linear((k - 0.5) / 255) in double, k = 1 .. 255."""
    s = (np.arange(256, dtype=np.float64) - 0.5) / 255.0
    lin = np.where(s <= 0.04045, s / 12.92, ((np.maximum(s, 0.0) + 0.055) / 1.055) ** 2.4)
    lin[0] = 0.0
    return lin


def colour(rgb, count=None):
    """(..., 3) float32 -> the input colour: rgb / count (0 where the count is 0) with a count plane, rgb without; then c > 0 ? c : 0."""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        if count is not None:
            n = np.asarray(count, np.uint32)[..., None]
            c = np.where(n > 0, rgb / n.astype(F), F(0))
        else:
            c = rgb
        return np.where(c > 0, c, F(0)).astype(F)


def lum(c):
    with np.errstate(all="ignore"):
        return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def bin_of(Y):
    """The bin of luminances > 0."""
    b = (np.ascontiguousarray(Y, F).view(np.uint32) >> 20).astype(np.int64) - BIAS
    return np.clip(b, 0, BINS - 1)


def edge(b):
    """Lower edge of bin b (b = 256: the last bin's upper edge, 4096)."""
    return np.array((int(b) + BIAS) << 20, np.uint32).view(F)[()]


def measure(rgb, count=None):
    """-> (hist: 256 uint32, n_dark)."""
    Y = lum(colour(rgb, count)).reshape(-1)
    lit = Y > 0
    return np.bincount(bin_of(Y[lit]), minlength=BINS).astype(np.uint32), int((~lit).sum())


def rank_bin(hist, rank):
    """The first bin whose running sum reaches rank, and the sum below it."""
    run = np.cumsum(hist.astype(np.uint64))
    b = int(np.searchsorted(run, np.uint64(rank), side="left"))
    return b, int(run[b]) - int(hist[b])


def solve(hist, n_dark, exposure=0.0, key=0.18, white_permille=995, white=0.0):
    """-> dict(n_lit, n_dark, y_median, y_white, exposure, white), the four floats float32."""
    hist = np.asarray(hist, np.uint32)
    N = int(hist.astype(np.uint64).sum())
    y_median = y_white = F(0)
    e, w = F(1), F(1)
    if N:
        rank_m, rank_w = (N + 1) // 2, max(1, (N * int(white_permille) + 999) // 1000)
        y_white = edge(rank_bin(hist, rank_w)[0] + 1)
        b, before = rank_bin(hist, rank_m)
        lo, hi = edge(b), edge(b + 1)
        t = (F(rank_m - before) - F(0.5)) / F(hist[b])
        y_median = F(lo + F(hi - lo) * t)
        with np.errstate(all="ignore"):
            e = F(F(key) / y_median)
    if exposure > 0:
        e = F(exposure)
    if N:
        with np.errstate(all="ignore"):
            w = np.maximum(F(e * y_white), F(1))
    if white > 0:
        w = F(white)
    return dict(n_lit=N, n_dark=int(n_dark), y_median=F(y_median), y_white=F(y_white), exposure=F(e), white=F(w))


def curve(op, c, exposure, white):
    """The input colour (..., 3) -> v in [0, 1], float32."""
    e, w = F(exposure), F(white)
    with np.errstate(all="ignore"):
        x = np.minimum(e * c, MAX).astype(F)
        if op == LINEAR:
            return np.minimum(x, F(1))
        if op == FILMIC:
            num = x * (F(2.51) * x + F(0.03))
            den = x * (F(2.43) * x + F(0.59)) + F(0.14)
            return np.minimum(num / den, F(1)).astype(F)
        L = lum(x)
        s = ((F(1) + L / F(w * w)) / (F(1) + L)).astype(F)
        return np.minimum(x * s[..., None], F(1)).astype(F)


def byte_of(T, v):
    """The number of k in 1 .. 255 with v >= T[k]."""
    return np.searchsorted(np.asarray(T, F)[1:], v, side="right").astype(np.uint32)


def encode(rgb, count, op, exposure, white, T):
    """-> (...) uint32 words, bytes R, G, B, 255 in memory order."""
    b = byte_of(T, curve(op, colour(rgb, count), exposure, white))
    return (b[..., 0] | (b[..., 1] << np.uint32(8)) | (b[..., 2] << np.uint32(16)) | np.uint32(0xFF000000)).astype(np.uint32)


def rgba_bytes(words):
    """(y, x) words -> (y, x, 4) uint8 as they lie in memory."""
    return np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(words.shape + (4,))


# ----------------------------------------------------------------------- inputs that sit on the byte thresholds
def _next(x, k):
    """k floats above (below for k < 0) a positive float32."""
    return (np.asarray(x, F).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F)


def threshold_inputs(op, exposure, white, T, others=None):
    """For k = 1 .. 255: the smallest positive float c with v(c) >= T[k] and the float just below it, found by bisection on the bit
    patterns (v is monotone in c).  others None: a grey pixel (c in all three channels); else (g, b) held fixed while c is the red
    channel.  -> (255, 2) float32: [k - 1] = (below, at).  The byte of red is k at `at` and k - 1 at `below` when the curve reaches
    T[k] at all (FILMIC and REINHARD saturate: rows that never reach it hold the largest finite float twice)."""
    T = np.asarray(T, F)

    def v_of(c):
        px = np.stack([c, c, c], -1) if others is None else np.stack([c, np.full_like(c, others[0]), np.full_like(c, others[1])], -1)
        return curve(op, px.astype(F), exposure, white)[..., 0]
    lo = np.full(255, 1, np.int64)                  # bits of the smallest denormal: v < T[k]
    hi = np.full(255, 0x7F7FFFFF, np.int64)         # the largest finite float
    want = T[1:]
    reach = v_of(hi.astype(np.uint32).view(F)) >= want
    for _ in range(32):
        mid = (lo + hi) // 2
        ok = v_of(mid.astype(np.uint32).view(F)) >= want
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid)
    at = hi.astype(np.uint32).view(F)
    below = _next(at, -1)
    out = np.stack([below, at], -1).astype(F)
    out[~reach] = np.finfo(F).max
    return out
