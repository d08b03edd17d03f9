"""MC-CNN's stereo method restated in numpy from its specification, independently of
csrc/sm_mcsgm.hpp: float32 arrays throughout, one numpy operation per rounded operation.  The CPU
twin must give the same values and the same NaN pattern (tests/test_mcsgm_host.py)."""
import math

import numpy as np

F = np.float32
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))  # r = p - q: from the left, right, above, below
CORRECT, MISMATCH, OCCLUDED = 0, 1, 2
WALKS = [(1, 0), (-1, 0), (0, 1), (0, -1)] + [(sx * ax, sy * ay) for ax, ay in ((1, 1), (1, 2), (2, 1))
                                              for sx in (1, -1) for sy in (1, -1)]


def normalise(img):
    """float32 image through the 256-entry table of §4.15; a constant image gives zeros."""
    g = np.asarray(img, dtype=np.int64)
    N = g.size
    sx, sxx = int(g.sum()), int((g * g).sum())
    q = N * sxx - sx * sx
    if q == 0:
        return np.zeros(g.shape, F)
    std = math.sqrt(float(q) / float(N * (N - 1)))
    tab = np.array([F((float(v * N - sx) / float(N)) / std) for v in range(256)], F)
    return tab[g]


def penalties(p):
    """(P1 of r0 / r1 by class, P1 of r2 / r3, P2), classes: both steps small, mixed, both large."""
    pi1, pi2, q1, q2, v = (F(getattr(p, k)) for k in ("pi1", "pi2", "sgm_q1", "sgm_q2", "sgm_v"))
    p1 = np.array([pi1, pi1 / q1, pi1 / q2], F)
    p2 = np.array([pi2, pi2 / q1, pi2 / q2], F)
    return p1, p1 / v, p2


def path(V, ta, tb, m, p, r, classes=None):
    """L_r of one image; classes (a list of three counters) collects the penalty classes met."""
    D, H, W = V.shape
    rx, ry = DIRS[r]
    p1h, p1v, p2 = penalties(p)
    p1 = p1h if rx else p1v
    thr = F(p.sgm_d)
    L = np.empty_like(V)
    delta = m + np.arange(D)
    nan = F(np.nan)
    n = W if rx else H
    with np.errstate(invalid="ignore"):
        for s in range(n):
            pos = s if rx + ry > 0 else n - 1 - s
            here = (slice(None), slice(None), pos) if rx else (slice(None), pos, slice(None))
            v = V[here]  # [D, other axis]
            if s == 0:
                L[here] = v
                continue
            prev = (slice(None), slice(None), pos - rx) if rx else (slice(None), pos - ry, slice(None))
            lq = L[prev]
            M = np.fmin.reduce(lq, axis=0)  # NaN where every plane is
            if rx:
                d1 = np.abs(ta[:, pos] - ta[:, pos - rx])  # [H]
                c0 = pos - delta  # [D]
                c1 = c0 - rx
                ok = (c0 >= 0) & (c0 < W) & (c1 >= 0) & (c1 < W)
                d2 = np.zeros((D, H), F)
                d2[ok] = np.abs(tb[:, c0[ok]] - tb[:, c1[ok]]).T
            else:
                d1 = np.abs(ta[pos] - ta[pos - ry])  # [W]
                c0 = np.arange(W)[None, :] - delta[:, None]  # [D, W]
                ok = (c0 >= 0) & (c0 < W)
                cc = np.clip(c0, 0, W - 1)
                d2 = np.where(ok, np.abs(tb[pos][cc] - tb[pos - ry][cc]), F(0)).astype(F)
            small1, small2 = (d1 < thr)[None, :], d2 < thr
            cls = np.where(small1 & small2, 0, np.where(~small1 & ~small2, 2, 1))
            P1, P2 = p1[cls], p2[cls]
            lqm = np.vstack([np.full((1, lq.shape[1]), nan, F), lq[:-1]])
            lqp = np.vstack([lq[1:], np.full((1, lq.shape[1]), nan, F)])
            e = M[None, :] + P2
            e = np.fmin(e, lq)
            e = np.fmin(e, lqm + P1)
            e = np.fmin(e, lqp + P1)
            res = (v - M[None, :]) + e
            dead = np.isnan(M)[None, :]
            L[here] = np.where(dead, v, res)
            if classes is not None:
                live = ~dead & ~np.isnan(v)
                for c in range(3):
                    classes[c] += int((live & (cls == c)).sum())
    return L


def aggregate(V, a, b, m, p, classes=None):
    """A of one image: V float32 [D, H, W], a / b uint8 [H, W]."""
    ta, tb = normalise(a), normalise(b)
    V = np.asarray(V, F)
    for _ in range(int(p.sgm_i)):
        l0, l1, l2, l3 = (path(V, ta, tb, m, p, r, classes) for r in range(4))
        V = ((l0 + l1) + (l2 + l3)) * F(0.25)
    return V


def wta(A):
    """Index of the smallest non-NaN plane (the first of equals), -1 where there is none."""
    dead = np.isnan(A)
    j = np.argmin(np.where(dead, np.inf, A), axis=0)
    return np.where(dead.all(axis=0), -1, j)


def disparity(AL, AR, a, m, p):
    """Every stage of one image, as a dict: wta_left, wta_right, status, filled (int32), subpixel,
    median, out (float32), and the bookkeeping the tests' conditions need (hits, guards)."""
    D, H, W = AL.shape
    inv = m - 1
    m_r = -(m + D) + 1
    jl, jr = wta(AL), wta(AR)
    dl = np.where(jl < 0, inv, m + jl).astype(np.int32)
    dr = np.where(jr < 0, inv, -(m_r + jr)).astype(np.int32)
    xs = np.arange(W)[None, :]
    rows = np.arange(H)[:, None]

    def consistent(delta):  # delta: [H, W] ints
        c = xs - delta
        ok = (c >= 0) & (c < W)
        r = dr[rows, np.clip(c, 0, W - 1)]
        return ok & (r != inv) & (np.abs(delta - r) <= 1)

    correct = (dl != inv) & consistent(dl)
    some = np.zeros((H, W), bool)
    for d in range(D):
        some |= consistent(np.full((H, W), m + d))
    status = np.where(correct, CORRECT, np.where(some & (dl != inv), MISMATCH, OCCLUDED)).astype(np.int32)

    filled = dl.copy()
    hits = np.full((H, W), -1)
    none_left = np.zeros((H, W), bool)
    for y in range(H):
        good = np.flatnonzero(status[y] == CORRECT)
        for x in range(W):
            if status[y, x] == OCCLUDED:
                left, right = good[good < x], good[good > x]
                none_left[y, x] = left.size == 0
                if left.size:
                    filled[y, x] = dl[y, left[-1]]
                elif right.size:
                    filled[y, x] = dl[y, right[0]]
            elif status[y, x] == MISMATCH:
                vals = []
                for dx, dy in WALKS:
                    xx, yy = x + dx, y + dy
                    while 0 <= xx < W and 0 <= yy < H:
                        if status[yy, xx] == CORRECT:
                            vals.append(int(dl[yy, xx]))
                            break
                        xx, yy = xx + dx, yy + dy
                hits[y, x] = len(vals)
                if vals:
                    filled[y, x] = sorted(vals)[len(vals) // 2]

    valid = filled != inv
    j = filled.astype(np.int64) - m
    sub = filled.astype(F)
    inner = valid & (j > 0) & (j < D - 1)
    jc = np.clip(j, 1, max(D - 2, 1))
    guards = {"edge_lo": valid & (j == 0), "edge_hi": valid & (j == D - 1)}
    if D >= 3:
        cm, c, cp = (AL[jc + k, rows, xs] for k in (-1, 0, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            den = F(2) * ((cp - F(2) * c) + cm)
            val = sub - (cp - cm) / den
        finite = ~(np.isnan(cm) | np.isnan(c) | np.isnan(cp))
        guards["nan"] = inner & ~finite
        guards["den0"] = inner & finite & (den == 0)
        use = inner & finite & (den != 0)
        sub = np.where(use, val, sub).astype(F)
    else:
        guards["nan"] = guards["den0"] = np.zeros((H, W), bool)

    med = sub.copy()
    for y in range(H):
        for x in range(W):
            if not valid[y, x]:
                continue
            y0, y1, x0, x1 = max(y - 2, 0), min(y + 3, H), max(x - 2, 0), min(x + 3, W)
            vals = np.sort(sub[y0:y1, x0:x1][valid[y0:y1, x0:x1]])
            med[y, x] = vals[vals.size // 2]

    sigma = float(F(p.blur_sigma))
    R = math.ceil(3.0 * sigma)
    ta = normalise(a)
    num, den = np.zeros((H, W), F), np.zeros((H, W), F)
    pad = lambda arr, fill: np.pad(arr, R, constant_values=fill)
    medp, tap, validp = pad(med, 0), pad(ta, 0), pad(valid, False)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            w = F(math.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma)))
            sl = (slice(R + dy, R + dy + H), slice(R + dx, R + dx + W))
            counts = validp[sl] & (np.abs(ta - tap[sl]) < F(p.blur_t))
            num = np.where(counts, num + w * medp[sl], num)
            den = np.where(counts, den + w, den)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(valid, num / den, med).astype(F)
    return {"wta_left": dl, "wta_right": dr, "status": status, "filled": filled.astype(np.int32), "subpixel": sub,
            "median": med, "out": out, "hits": hits, "none_left": none_left, "guards": guards}
