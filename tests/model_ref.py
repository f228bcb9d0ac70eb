"""numpy restatement of include/pvmodel.h (the definition the device is held to): extent with the
centroid's lane order, farthest points with the tie rule, the all-pairs diameter.  Everything is
fp64 with every operation rounded; nothing here is fast.

* :func:`model_rows`      the skip rule: a model's rows, or None
* :func:`extent`          box, centroid (lane order), count
* :func:`farthest_points` the three start modes; a tie goes to the lowest index
* :func:`diameter`        sqrt of the largest d2 over i <= j
* :func:`table_*`         the same over a whole table (points, off, max_pn)
"""
import numpy as np

SUM_LANES = 256
MAX_K = 1024
BLOCK_MAX_PN = 12288
CHUNK = 8192
TILE = 256
START_CENTROID, START_CENTROID_KEPT, START_INDEX = 0, 1, 2


def widen(points):
    return np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)


def present(v):
    return np.isfinite(v).all(1)


def d2(v, q):
    """((dx dx + dy dy) + dz dz) of every row of v against the point q."""
    with np.errstate(all="ignore"):
        dx, dy, dz = v[:, 0] - q[0], v[:, 1] - q[1], v[:, 2] - q[2]
        return (dx * dx + dy * dy) + dz * dz


def model_rows(points, off, m, max_pn):
    """The rows of model m as f64 [n, 3], or None for a skipped model."""
    total = np.asarray(points).reshape(-1, 3).shape[0]
    lo, hi = int(off[m]), int(off[m + 1])
    if not (0 <= lo <= hi <= total) or hi - lo > max_pn:
        return None
    return widen(np.asarray(points).reshape(-1, 3)[lo:hi])


def lane_sum(x):
    """The header's order: lane j adds x[j], x[j + 256], ... from +0.0, then the halving tree."""
    lane = np.zeros(SUM_LANES)
    for j in range(min(SUM_LANES, x.shape[0])):
        s = 0.0
        for e in x[j::SUM_LANES]:
            s = s + float(e)
        lane[j] = s
    s = SUM_LANES // 2
    while s:
        lane[:s] = lane[:s] + lane[s:2 * s]
        s //= 2
    return float(lane[0])


def extent(v):
    """v f64 [n, 3] or None -> dict(bbox_min, bbox_max, centroid f64 [3], count)."""
    nan3 = np.full(3, np.nan)
    if v is None:
        return dict(bbox_min=nan3, bbox_max=nan3.copy(), centroid=nan3.copy(), count=0)
    ok = present(v)
    n = int(ok.sum())
    if n == 0:
        return dict(bbox_min=nan3, bbox_max=nan3.copy(), centroid=nan3.copy(), count=0)
    z = np.where(ok[:, None], v, 0.0)                      # an absent point contributes +0.0
    cen = np.array([lane_sum(z[:, e]) / float(n) for e in range(3)])
    return dict(bbox_min=v[ok].min(0) + 0.0, bbox_max=v[ok].max(0) + 0.0, centroid=cen, count=n)


def argmax_low(x, ok):
    """The arg-max of x over ok; a tie goes to the lowest index (np.argmax returns the first)."""
    return int(np.argmax(np.where(ok, x, -1.0)))


def farthest_points(v, k, start=START_CENTROID, start_idx=None, centroid=None):
    """-> dict(idx i32 [k], picked f64 [k, 3], pick_d2 f64 [k]).  centroid: extent(v)'s, if the
    caller has it already."""
    dead = dict(idx=np.full(k, -1, np.int32), picked=np.full((k, 3), np.nan), pick_d2=np.full(k, np.nan))
    if v is None or v.shape[0] == 0:
        return dead
    ok = present(v)
    if not ok.any():
        return dead
    if start == START_INDEX:
        s0 = int(start_idx)
        if not (0 <= s0 < v.shape[0]) or not ok[s0]:
            return dead
        pick, won = [s0], [np.inf]
        md = np.full(v.shape[0], np.inf)
    else:
        key = d2(v, extent(v)["centroid"] if centroid is None else centroid)
        pick = [argmax_low(key, ok)]
        won = [key[pick[0]]]
        md = key.copy() if start == START_CENTROID_KEPT else np.full(v.shape[0], np.inf)
    md = np.minimum(md, np.where(ok, d2(v, v[pick[0]]), np.inf))
    while len(pick) < k:
        i = argmax_low(md, ok)
        pick.append(i)
        won.append(md[i])
        md = np.minimum(md, np.where(ok, d2(v, v[i]), np.inf))
    return dict(idx=np.array(pick, np.int32), picked=v[pick], pick_d2=np.array(won, np.float64))


def diameter(v, block=1024):
    """sqrt(max over i <= j of d2(p_i, p_j)) over the finite points; NaN for none."""
    if v is None:
        return np.nan
    p = v[present(v)]
    if p.shape[0] == 0:
        return np.nan
    best = 0.0
    for a in range(0, p.shape[0], block):
        q = p[a:a + block]
        dx, dy, dz = (q[:, None, e] - p[None, a:, e] for e in range(3))
        best = max(best, float(((dx * dx + dy * dy) + dz * dz).max()))
    return float(np.sqrt(best))


# ---- over a table -------------------------------------------------------------------------------------
def table_extent(points, off, max_pn):
    es = [extent(model_rows(points, off, m, max_pn)) for m in range(len(off) - 1)]
    return dict(bbox_min=np.array([e["bbox_min"] for e in es]).reshape(-1, 3),
                bbox_max=np.array([e["bbox_max"] for e in es]).reshape(-1, 3),
                centroid=np.array([e["centroid"] for e in es]).reshape(-1, 3),
                count=np.array([e["count"] for e in es], np.int32))


def table_farthest_points(points, off, max_pn, k, start=START_CENTROID, start_idx=None, centroid=None):
    """centroid: table_extent's, if the caller has it already."""
    rs = [farthest_points(model_rows(points, off, m, max_pn), k, start, None if start_idx is None else start_idx[m],
                          None if centroid is None else centroid[m])
          for m in range(len(off) - 1)]
    return dict(idx=np.array([r["idx"] for r in rs], np.int32).reshape(-1, k),
                picked=np.array([r["picked"] for r in rs]).reshape(-1, k, 3),
                pick_d2=np.array([r["pick_d2"] for r in rs]).reshape(-1, k))


def table_diameter(points, off, max_pn):
    return np.array([diameter(model_rows(points, off, m, max_pn)) for m in range(len(off) - 1)])
