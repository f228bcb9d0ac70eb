"""include/pvloss.h restated in numpy float64: the yardstick of the loss tests.

Inputs are taken as they are (already rounded to the kind the device gets) and widened to float64;
every sum is a float64 sum.  ``seg`` is [b, ncls+1, H, W]; ``vertex`` and ``target`` are the logical
[b, H, W, ncls*vn, 2] (``logical`` makes that view of the network's [b, 2*ncls*vn, H, W]); ``label``
is any integer [b, H, W].  Either term may be None.
"""
import numpy as np


def logical(field, ncls):
    """The [b, H, W, C, 2] view of a field in either layout."""
    field = np.asarray(field)
    if field.ndim == 5:
        return field
    b, c2, H, W = field.shape
    return field.transpose(0, 2, 3, 1).reshape(b, H, W, c2 // 2, 2)


def network(field5):
    """[b, H, W, C, 2] -> a contiguous [b, 2 C, H, W]."""
    b, H, W, C, _ = field5.shape
    return np.ascontiguousarray(field5.reshape(b, H, W, 2 * C).transpose(0, 3, 1, 2))


def _weights(label, ncls, vn):
    """[b, H, W, ncls*vn] bool: the elements of a pixel that its label selects."""
    lab = np.asarray(label).astype(np.int64)
    cls = np.arange(ncls * vn) // vn                                   # the class of each channel
    return (lab[..., None] - 1) == cls[None, None, None, :]


def _sl1(d, sigma):
    s2 = float(sigma) * float(sigma)
    return np.where(np.abs(d) < 1.0 / s2, 0.5 * s2 * d * d, np.abs(d) - 0.5 / s2)


def _sl1_slope(d, sigma):
    s2 = float(sigma) * float(sigma)
    return np.where(np.abs(d) < 1.0 / s2, s2 * d, np.sign(d))


def _softmax_parts(seg):
    z = np.asarray(seg).astype(np.float64)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    return z, m, e, s


def forward(seg, vertex, target, label, ncls, vn, sigma=1.0):
    """-> {"loss_seg" [b], "loss_vertex" [b] (float64; None for an absent term), "fg" [b],
    "counts" [b, ncls, 3] = (tp, fp, fn) (int64; None without seg)}."""
    lab = np.asarray(label).astype(np.int64)
    b, H, W = lab.shape
    out = {"loss_seg": None, "loss_vertex": None, "counts": None}
    fgm = (lab >= 1) & (lab <= ncls)
    out["fg"] = fgm.reshape(b, -1).sum(1).astype(np.int64)
    if seg is not None:
        z, m, e, s = _softmax_parts(seg)
        lse = (m + np.log(s))[:, 0]
        inr = (lab >= 0) & (lab <= ncls)
        zl = np.take_along_axis(z, np.where(inr, lab, 0)[:, None], 1)[:, 0]
        ce = np.where(inr, lse - zl, 0.0)
        out["loss_seg"] = ce.reshape(b, -1).sum(1) / float(H * W)
        pred = np.argmax(z, 1)                                         # the lowest index of a tie
        counts = np.zeros((b, ncls, 3), np.int64)
        for c in range(ncls):
            p, t = pred == c + 1, lab == c + 1
            counts[:, c, 0] = (p & t).reshape(b, -1).sum(1)
            counts[:, c, 1] = (p & ~t).reshape(b, -1).sum(1)
            counts[:, c, 2] = (~p & t).reshape(b, -1).sum(1)
        out["counts"] = counts
    if vertex is not None:
        w = _weights(lab, ncls, vn)[..., None]
        with np.errstate(invalid="ignore"):
            d = np.where(w, logical(vertex, ncls).astype(np.float64) - logical(target, ncls).astype(np.float64), 0.0)
        S = np.where(w, _sl1(d, sigma), 0.0).reshape(b, -1).sum(1)
        out["loss_vertex"] = S / (2.0 * vn * out["fg"] + 1e-3)
    return out


def backward(seg, vertex, target, label, ncls, vn, sigma=1.0, g_seg=None, g_vertex=None):
    """-> (grad_seg [b, ncls+1, H, W], grad_vertex [b, H, W, ncls*vn, 2]) in float64, None for an absent
    term; g_seg, g_vertex [b] are the upstream gradients of the per-image losses (default 1)."""
    lab = np.asarray(label).astype(np.int64)
    b, H, W = lab.shape
    gs = gv = None
    if seg is not None:
        g = np.ones(b) if g_seg is None else np.asarray(g_seg, np.float64)
        z, m, e, s = _softmax_parts(seg)
        inr = (lab >= 0) & (lab <= ncls)
        onehot = np.arange(ncls + 1)[None, :, None, None] == lab[:, None]
        gs = np.where(inr[:, None], (e / s - onehot) * g[:, None, None, None] / float(H * W), 0.0)
    if vertex is not None:
        g = np.ones(b) if g_vertex is None else np.asarray(g_vertex, np.float64)
        fg = ((lab >= 1) & (lab <= ncls)).reshape(b, -1).sum(1)
        w = _weights(lab, ncls, vn)[..., None]
        with np.errstate(invalid="ignore"):
            d = np.where(w, logical(vertex, ncls).astype(np.float64) - logical(target, ncls).astype(np.float64), 0.0)
        scale = g / (2.0 * vn * fg + 1e-3)
        gv = np.where(w, _sl1_slope(d, sigma) * scale[:, None, None, None, None], 0.0)
    return gs, gv
