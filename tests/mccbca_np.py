"""Cross-based cost aggregation restated in numpy from its specification,
independently of csrc/sm_mccbca.hpp: float32 arrays throughout, one numpy operation per rounded
operation, loops over the offset k and never over pixels.  The CPU twin must give the same values
and the same NaN pattern (tests/test_mccbca_host.py)."""
import numpy as np

from mcsgm_np import normalise

F = np.float32
STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # (sx, sy): left, right, up, down
CAP, BORDER, TAU = 0, 1, 2  # why an arm stopped


def arms(img, l1, tau1, reasons=None):
    """uint8 [4, H, W]: left, right, up, down.  reasons (a list) receives, per direction, an int
    map of why each arm stopped: the cap L1, the border, tau1."""
    t = normalise(img)
    H, W = t.shape
    tau = F(tau1)
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((4, H, W), np.uint8)
    for s, (sx, sy) in enumerate(STEPS):
        n = np.zeros((H, W), np.int64)
        alive = np.ones((H, W), bool)
        why = np.full((H, W), CAP)
        for k in range(1, l1):
            xx, yy = xs + k * sx, ys + k * sy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            other = t[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            close = np.abs(t - other) < tau
            why[alive & ~inside] = BORDER
            why[alive & inside & ~close] = TAU
            alive &= inside & close
            n[alive] = k
        out[s] = n
        if reasons is not None:
            reasons.append(why)
    return out


def cross(C, a, b, m, l1, tau1, stats=None):
    """One iteration C' = cross(C, a, b, m) of one image; stats (a dict) receives the combined arms
    and the mask of the cells that exist."""
    C = np.asarray(C, F)
    D, H, W = C.shape
    la, ra, ua, da = (x.astype(np.int64) for x in arms(a, l1, tau1))
    lb, rb, ub, db = (x.astype(np.int64) for x in arms(b, l1, tau1))
    out = C.copy()
    xs = np.arange(W)
    ys = np.arange(H)[:, None]
    h = l1 - 1
    if stats is not None:
        stats.update(exists=np.zeros(C.shape, bool), arm_a=np.zeros((4,) + C.shape, np.int64), arm_b=np.zeros((4,) + C.shape, np.int64))
    with np.errstate(invalid="ignore"):
        for d in range(D):
            xb = xs - (m + d)
            ok = (xb >= 0) & (xb < W)
            if not ok.any():
                continue
            cb = np.clip(xb, 0, W - 1)
            l, r = np.minimum(la, lb[:, cb]), np.minimum(ra, rb[:, cb])
            u, w = np.minimum(ua, ub[:, cb]), np.minimum(da, db[:, cb])
            # S: the terms C[x - l + j], j = 0 .. l + r, ascending, from the first one
            S = C[d][ys, np.clip(xs - l, 0, W - 1)]
            for j in range(1, 2 * h + 1):
                use = j <= l + r
                term = C[d][ys, np.clip(xs - l + j, 0, W - 1)]
                S = np.where(use, S + term, S)
            nh = l + r + 1
            # T: the terms S[y - u + j], j = 0 .. u + w; N likewise
            T = S[np.clip(ys - u, 0, H - 1), xs]
            N = nh[np.clip(ys - u, 0, H - 1), xs]
            for j in range(1, 2 * h + 1):
                use = j <= u + w
                row = np.clip(ys - u + j, 0, H - 1)
                T = np.where(use, T + S[row, xs], T)
                N = np.where(use, N + nh[row, xs], N)
            res = T / N.astype(F)
            out[d][:, ok] = res[:, ok]
            if stats is not None:
                stats["exists"][d][:, ok] = True
                for i, (pa, pb) in enumerate(((la, lb), (ra, rb), (ua, ub), (da, db))):
                    stats["arm_a"][i, d] = pa
                    stats["arm_b"][i, d] = pb[:, cb]
    return out


def aggregate(vol, a, b, m, l1, tau1, iterations=1):
    out = np.asarray(vol, F)
    for _ in range(iterations):
        out = cross(out, a, b, m, l1, tau1)
    return out
