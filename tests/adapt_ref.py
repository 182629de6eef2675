"""numpy restatement of the adaptive tile rule (include/rgk.h rgk_adapt_select, rgk_amd/csrc/rgk_adapt.h) and of the round fold
(rgk_round_fold_device).  The rule is in double with the tiles added one after the other in row-major order -- a Python loop, not
np.sum, whose pairwise order would differ in the last place -- and the comparisons are the ones the header writes."""
import numpy as np

TILE_DT = np.dtype([("sum_var", "f8"), ("sum_sq", "f8"), ("n_estimable", "u8")])


def select(tiles, visits, target, min_visits):
    """tiles: structured array (any shape, taken row-major), visits: same number of entries -> (live bool (n,), n_live, done)."""
    t = np.asarray(tiles, dtype=TILE_DT).reshape(-1)
    v = np.asarray(visits).reshape(-1)
    SV = SQ = 0.0
    NE = 0
    for k in range(t.size):
        SV += float(t["sum_var"][k])
        SQ += float(t["sum_sq"][k])
        NE += int(t["n_estimable"][k])
    t32 = float(np.float32(target))
    allowance = (t32 * t32) * SQ
    done = NE > 0 and SV <= allowance
    live = np.zeros(t.size, bool)
    for k in range(t.size):
        ne = int(t["n_estimable"][k])
        live[k] = bool(v[k] < min_visits) or ne == 0 or float(t["sum_var"][k]) > allowance * (float(ne) / float(NE))
    n_live = int(live.sum())
    return live, n_live, bool(done or n_live == 0)


def fold(tiles, to_half, round_rgb, round_count, total_rgb, total_count, half_rgb, half_count):
    """The six planes after rgk_round_fold_device (copies; the arguments are not changed).  tiles: (x0, x1, y0, y1) each."""
    out = [np.array(a, copy=True) for a in (round_rgb, round_count, total_rgb, total_count, half_rgb, half_count)]
    rr, rc, tr, tc, hr, hc = out
    for (x0, x1, y0, y1), h in zip(tiles, to_half):
        s = (slice(y0, y1), slice(x0, x1))
        tr[s] = tr[s] + rr[s]
        tc[s] = tc[s] + rc[s]
        if h:
            hr[s] = hr[s] + rr[s]
            hc[s] = hc[s] + rc[s]
        rr[s] = 0
        rc[s] = 0
    return out
