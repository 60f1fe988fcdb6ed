"""The float64 numpy restatement of the per-class box head (include/frcnn_hip_box.h; csrc/box_head.hip): the class-source
rules, the three kernels, and the error bounds the tests hold the device to.  Nothing here looks at the device's results."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def first_maximum(row):
    """frcnn_cnet_decode's comparison on one row of log-probabilities: `best` starts at column 0 and moves only on a strict >
    (so a NaN in column 0 stays, a NaN elsewhere is never taken, ties keep the lowest column) -> the 0-based column"""
    row = np.asarray(row, dtype=np.float32)
    best = 0
    for j in range(1, row.shape[0]):
        if row[j] > row[best]:       # (a comparison with a NaN is False)
            best = j
    return best


def select(R, C, kind, classes=None, n_fg=0, lsm=None):
    """-> sel int32[R]: the class each row uses, 0 for none.  kind "int": classes[r] for r < n_fg, background behind; "float": an
    fp32 1-based class per row, (int) of it where 1 <= it <= C as floats; "argmax": the first maximum of lsm's row, plus 1.
    Anything outside 1 ... C -- the background, garbage, a NaN -- is 0."""
    sel = np.zeros(R, np.int64)
    if kind == "int":
        cl = np.asarray(classes, dtype=np.int32).reshape(-1)
        sel[:n_fg] = cl[:n_fg]
    elif kind == "float":
        t = np.asarray(classes, dtype=np.float32).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok = (t >= np.float32(1.0)) & (t <= np.float32(C))
        sel[ok] = np.trunc(t[ok].astype(np.float64)).astype(np.int64)
    elif kind == "argmax":
        lsm = np.asarray(lsm, dtype=np.float32)
        for r in range(R):
            sel[r] = first_maximum(lsm[r]) + 1
    else:
        raise ValueError(kind)
    sel[(sel < 1) | (sel > C)] = 0
    return sel.astype(np.int32)


def forward(x, W, b, sel):
    """-> (out float64[R][4], mag float64[R][4] = |b| + sum |x w|: what the forward bound scales with)"""
    x, W, b = (np.asarray(a, dtype=np.float64) for a in (x, W, b))
    R, nf = x.shape
    out, mag = np.zeros((R, 4)), np.zeros((R, 4))
    for r in range(R):
        c = int(sel[r])
        if c == 0:
            continue
        w4 = W[4 * (c - 1):4 * c]
        out[r] = w4 @ x[r] + b[4 * (c - 1):4 * c]
        mag[r] = np.abs(w4) @ np.abs(x[r]) + np.abs(b[4 * (c - 1):4 * c])
    return out, mag


def input_gradient(g, W, sel):
    """-> (gfeat float64[R][nf], mag = sum_j |g_j w_jk|); rows with sel = 0 are zero whatever g holds"""
    g, W = np.asarray(g, dtype=np.float64), np.asarray(W, dtype=np.float64)
    R, nf = g.shape[0], W.shape[1]
    out, mag = np.zeros((R, nf)), np.zeros((R, nf))
    for r in range(R):
        c = int(sel[r])
        if c == 0:
            continue
        w4 = W[4 * (c - 1):4 * c]
        out[r] = g[r] @ w4
        mag[r] = np.abs(g[r]) @ np.abs(w4)
    return out, mag


def weight_gradient(g, x, sel, C, gW0, gb0):
    """-> dict(gW, gb: the prior gradients plus the sums over each class's rows (float64), magW, magb: |G0| + sum |g x|, n:
    rows per class int[C], touched: bool[C] -- the classes with a row; the rows of the others must stay as they were)"""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    gW, gb = np.asarray(gW0, dtype=np.float64).copy(), np.asarray(gb0, dtype=np.float64).copy()
    magW, magb = np.abs(gW), np.abs(gb)
    n = np.zeros(C, np.int64)
    for c in range(1, C + 1):
        rows = np.nonzero(np.asarray(sel) == c)[0]
        n[c - 1] = len(rows)
        if not len(rows):
            continue
        gW[4 * (c - 1):4 * c] += g[rows].T @ x[rows]
        gb[4 * (c - 1):4 * c] += g[rows].sum(0)
        magW[4 * (c - 1):4 * c] += np.abs(g[rows]).T @ np.abs(x[rows])
        magb[4 * (c - 1):4 * c] += np.abs(g[rows]).sum(0)
    return dict(gW=gW, gb=gb, magW=magW, magb=magb, n=n, touched=n > 0)


# ---- the bounds (u = 2^-24), from the operation counts ---------------------------------------------------------------------------
# forward: nf products (one rounding each, or none when fused into the add), nf - 1 additions of the dot product in any order,
#   one addition of the bias: every term passes through at most nf + 1 roundings, so the error is at most
#   ((1 + u)^(nf + 1) - 1) (|b| + sum |x w|) <= (nf + 2) u (|b| + sum |x w|) while (nf + 2) u << 1.
# input gradient: 4 products and 3 additions in a fixed order: at most 4 roundings on a term -> 5 u sum_j |g_j w_jk|.
# weight gradient: n_c products, n_c - 1 additions among them, one addition to the prior gradient G0 -> (n_c + 2) u (|G0| + sum).
def forward_bound(nf, mag):
    return (nf + 2) * U * mag


def input_gradient_bound(mag):
    return 5 * U * mag


def weight_gradient_bound(n_rows, mag):
    """n_rows: rows of the element's class (int per class, repeated over the class's four rows by the caller)"""
    return (n_rows + 2) * U * mag
