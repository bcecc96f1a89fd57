"""Referee of the device-side evaluation (gsn_amd/evaluation.py, csrc/evaluate.hip): the masked mean losses of the reference's --loss_fn
kinds and their gradients in float64, with the absolute scale against which an error is read (the sum of the magnitudes of the parts that
are added or subtracted: a result that cancels says nothing about the error of its parts), and ROC-AUC / average precision from exact
integer run statistics by a sort.  numpy only."""
import math

import numpy as np

KINDS = ("BCEWithLogitsLoss", "L1Loss", "MSELoss", "CrossEntropyLoss")


def masked_loss_ref(kind, y_hat, y, grad_out=1.0):
    """``(loss, loss_scale, grad, grad_scale)``: float, float, float64 arrays of y_hat's shape.  Element-wise kinds: y float with NaN =
    unlabelled, viewed to y_hat's shape.  CrossEntropyLoss: y integer [rows]; a target outside [0, C) gives a NaN loss and a zero row."""
    x = np.asarray(y_hat, dtype=np.float64)
    g = float(grad_out)
    if kind == "CrossEntropyLoss":
        t = np.asarray(y).reshape(-1).astype(np.int64)
        rows, n_cls = x.shape
        ok = (t >= 0) & (t < n_cls)
        tc = np.where(ok, t, 0)
        m = x.max(axis=1)
        e = np.exp(x - m[:, None])
        s = e.sum(axis=1)
        xt = x[np.arange(rows), tc]
        elem = np.where(ok, m + np.log(s) - xt, np.nan)
        escale = np.abs(m) + np.log(s) + np.abs(xt)
        onehot = np.zeros_like(x)
        onehot[np.arange(rows), tc] = 1.0
        d = np.where(ok[:, None], e / s[:, None] - onehot, 0.0)
        dscale = np.where(ok[:, None], e / s[:, None] + onehot, 0.0)
        n = rows
        loss = float(elem.sum() / n) if n else math.nan
        return loss, (float(escale.sum() / n) if n else 0.0), g * d / max(n, 1), abs(g) * dscale / max(n, 1)
    yy = np.asarray(y, dtype=np.float64).reshape(x.shape)
    lab = ~np.isnan(yy)
    y0 = np.where(lab, yy, 0.0)
    if kind == "BCEWithLogitsLoss":
        a, b, c = np.maximum(x, 0.0), x * y0, np.log1p(np.exp(-np.abs(x)))
        elem, escale = a - b + c, a + np.abs(b) + c
        ex = np.exp(-np.abs(x))
        sig = np.where(x >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))
        d, dscale = sig - y0, sig + np.abs(y0)
    elif kind == "L1Loss":
        elem = np.abs(x - y0)
        escale = elem
        d = np.sign(x - y0)
        dscale = np.abs(d)
    elif kind == "MSELoss":
        elem = (x - y0) ** 2
        escale = elem
        d = 2.0 * (x - y0)
        dscale = np.abs(d)
    else:
        raise NotImplementedError(kind)
    n = int(lab.sum())
    if n == 0:
        return math.nan, 0.0, np.zeros_like(x), np.zeros_like(x)
    return (float(elem[lab].sum() / n), float(escale[lab].sum() / n), np.where(lab, g * d / n, 0.0), np.where(lab, abs(g) * dscale / n, 0.0))


FP32_TINY = 2.0 ** -149          # the smallest positive fp32 number: an fp32 result cannot be closer than this to a value below it


def normalised_error(x, ref, scale, tiny=0.0):
    """max |x - ref| / scale (0 for an empty array; where the scale is 0 the value must be exact; a NaN referee wants a NaN).  ``tiny``: an
    absolute difference up to it counts as none (FP32_TINY for fp32 results: a softmax of 1e-90 is stored as 0)."""
    x, ref, scale = (np.asarray(v, dtype=np.float64).reshape(-1) for v in np.broadcast_arrays(x, ref, scale))
    if ref.size == 0:
        return 0.0
    both_nan = np.isnan(x) & np.isnan(ref)
    d = np.where(both_nan, 0.0, np.abs(x - ref))
    d = np.where(np.isnan(d), np.inf, d)
    d = np.where(d <= tiny, 0.0, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(e.max())


def rank_ref(score, label):
    """One column: ``dict(n, n_pos, u2, auc, ap)`` of fp32 scores against labels 0 / 1 / NaN (unlabelled rows are left out).  u2 is the
    exact integer  sum over runs of equal scores of  pos * (2 * negatives below + negatives in the run)  = 2 #(p > n) + #(p == n) over all
    (positive, negative) pairs; auc = u2 / (2 n_pos n_neg) (None with one class); ap = the sum over runs from the highest score down of
    (pos / n_pos) * tp / (tp + fp) (None without a positive)."""
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    label = np.asarray(label, dtype=np.float64).reshape(-1)
    lab = ~np.isnan(label)
    s, l = score[lab].astype(np.float64), label[lab]
    n = int(lab.sum())
    if n == 0:
        return dict(n=0, n_pos=0, u2=0, auc=None, ap=None)
    _, inv = np.unique(s, return_inverse=True)               # (-0.0 == +0.0: one value)
    pos_r = np.bincount(inv, weights=(l == 1)).astype(np.int64)
    neg_r = np.bincount(inv, weights=(l == 0)).astype(np.int64)
    n_pos, n_neg = int(pos_r.sum()), int(neg_r.sum())
    neg_below = np.cumsum(neg_r) - neg_r
    u2 = sum(int(p) * (2 * int(b) + int(q)) for p, b, q in zip(pos_r, neg_below, neg_r) if p)
    auc = u2 / (2 * n_pos * n_neg) if n_pos and n_neg else None
    ap = None
    if n_pos:
        pd, td = pos_r[::-1], (pos_r + neg_r)[::-1]
        tp, tot = np.cumsum(pd), np.cumsum(td)
        ap = 0.0
        for p, a, b in zip(pd, tp, tot):
            if p:
                ap += (float(p) / n_pos) * (float(a) / float(b))
    return dict(n=n, n_pos=n_pos, u2=u2, auc=auc, ap=ap)


def u2_brute(score, label):
    """2 #(p > n) + #(p == n) over all (positive, negative) pairs of the labelled rows"""
    score = np.asarray(score, dtype=np.float32).reshape(-1).astype(np.float64)
    label = np.asarray(label, dtype=np.float64).reshape(-1)
    p, q = score[label == 1], score[label == 0]
    gt = eq = 0
    for lo in range(0, len(p), 512):
        blk = p[lo:lo + 512, None]
        gt += int((blk > q[None, :]).sum())
        eq += int((blk == q[None, :]).sum())
    return 2 * gt + eq
