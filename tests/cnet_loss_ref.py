"""The float64 numpy restatement of frcnn_cnet_loss_rows (include/frcnn_hip_loss.h; csrc/cnet_loss.hip), the case tables of its
tests and the bounds those tests hold the device to.

The restatement performs the header's operations in the header's order on IEEE doubles, one at a time (numpy never fuses a
multiply with an add), and rounds every stored float once.  Where a row's value involves no exp / expm1 / pow -- the NLL, the
smoothed NLL, SmoothL1, and every special value -- the device must give the same BITS.  Elsewhere the two differ by what the
transcendental functions differ by; the bounds below follow from the operation count:

  ULP = 2^-52, the largest relative size of one unit in the last place of a double.
  The device's double-precision exp and expm1 are within 3 ulp and pow within 16 ulp (the OpenCL limits, which the ROCm device
  library documents it meets); the host's are within 1.  So exp / expm1 results differ by at most E1 = 4 ULP relative, pow results
  of equal arguments by at most EP = 17 ULP relative.
  A stored float differs by at most the spacing of floats at the value (two values that close may round to neighbours) plus the
  fp64 difference: tol32(v, e64) = spacing_f32(|v|) + e64.

  focal (gamma = g):  q = -expm1(lp) carries E1; pow(q, g) carries g E1 + EP; the products with w and lp one ULP each:
      |d cls| <= (g E1 + EP + 2 ULP) |cls|                                                                        (focal_cls_err)
      the target gradient w (-q^g + x) / R, x = g q^(g-1) (1 - q) lp: q^g as above; q^(g-1) carries |g-1| E1 + EP; 1 - q has the
      ABSOLUTE error E1 q, which enters x as g q^(g-1) E1 q |lp| = g E1 q^g |lp|; four more roundings:
      |d grad| <= w / R * ((g E1 + EP + 4 ULP) q^g + (|g-1| E1 + EP + 4 ULP) |x| + g E1 q^g |lp|)               (focal_grad_err)
  giou:  with M = the largest |corner| or |origin| of the two boxes, S = the largest side of the enclosing box and m = the
      smallest side of the two boxes: a side from exp carries E1 S, a far corner one rounding more, a difference of corners one
      more, for both boxes: every side (own, intersection, enclosing) is off by at most e_s = 12 ULP (M + S).
      |dI| <= 2 S e_s, |dAp| + |dAt| <= 4 S e_s, so |dU| <= 6 S e_s and |dC| <= 2 S e_s; U and C are at least m^2, I / U and U / C
      at most 1:  |d(I/U)| <= (|dI| + |dU|) / U <= 8 S e_s / m^2, |d(U/C)| <= (|dU| + |dC|) / C <= 8 S e_s / m^2, three roundings:
      |d box| <= 16 S e_s / m^2 + 3 ULP * 2                                                                       (giou_box_err)
      an edge gradient is four products (edge term) * (coefficient): edge terms are sides, at most S, off by 2 e_s (gU: two
      of them); coefficients 1/U, (I/U)/U, 1/C, (U/C)/C are at most 1/m^2 and off by at most 14 S e_s / m^4:
      |d g_edge| <= 4 (2 e_s / m^2 + 2 S * 14 S e_s / m^4);  a delta's gradient is a sum of two of them or one times a side
      (factor max(1, S), and E1 of the side on the value itself):
      |d crdelta| <= box_weight * (2 max(1, S) * 4 (2 / m^2 + 28 S^2 / m^4) e_s) + 8 ULP |crdelta|               (giou_grad_err)
The selections (min / max, iw > 0, the clamp) are discontinuous: the cases keep clear of them except where a tie holds exactly
on both sides (equal inputs give equal exp results on one device, and the origins involve no exp)."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
ULP = 2.0 ** -52
E1 = 4 * ULP
EP = 17 * ULP
K = math.log(1000.0 / 16.0)
assert K.hex() == "0x1.08a691a12e2a9p+2"          # the constant of cnet_loss.hip

DEFAULT = dict(cls="nll", gamma=2.0, alpha=None, label_smoothing=0.0, box="smooth_l1", beta=1.0, box_weight=10.0)


def desc(**kw):
    d = dict(DEFAULT)
    d.update(kw)
    return d


def spacing32(v):
    v = np.abs(np.asarray(v, F32))
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(v), np.spacing(v), 0.0).astype(F64)


def giou_row(c, t):
    """c, t: four doubles each (prediction, target deltas) -> box, d box / d c (4), and (M, S, m) of the error bound"""
    c = [F64(v) for v in c]; t = [F64(v) for v in t]
    in2, in3 = c[2] <= K, c[3] <= K
    pw, ph = np.exp(c[2] if in2 else F64(K)), np.exp(c[3] if in3 else F64(K))
    x0, y0 = c[0], c[1]
    x1, y1 = x0 + pw, y0 + ph
    tx0, ty0 = t[0], t[1]
    tx1, ty1 = tx0 + np.exp(t[2]), ty0 + np.exp(t[3])
    pw_, ph_ = x1 - x0, y1 - y0
    Ap, At = pw_ * ph_, (tx1 - tx0) * (ty1 - ty0)
    six0, six1, siy0, siy1 = x0 >= tx0, x1 <= tx1, y0 >= ty0, y1 <= ty1
    iw = (x1 if six1 else tx1) - (x0 if six0 else tx0)
    ih = (y1 if siy1 else ty1) - (y0 if siy0 else ty0)
    has = bool(iw > 0.0 and ih > 0.0)
    I = iw * ih if has else F64(0.0)
    sex0, sex1, sey0, sey1 = x0 <= tx0, x1 >= tx1, y0 <= ty0, y1 >= ty1
    ew = (x1 if sex1 else tx1) - (x0 if sex0 else tx0)
    eh = (y1 if sey1 else ty1) - (y0 if sey0 else ty0)
    Cc = ew * eh
    U = (Ap + At) - I
    iou, fill = I / U, U / Cc
    a, b, cc, d = F64(1.0) / U, iou / U, F64(1.0) / Cc, fill / Cc
    z = F64(0.0)
    gI = [-ih if has and six0 else z, -iw if has and siy0 else z, ih if has and six1 else z, iw if has and siy1 else z]
    gA = [-ph_, -pw_, ph_, pw_]
    gC = [-eh if sex0 else z, -ew if sey0 else z, eh if sex1 else z, ew if sey1 else z]
    g = []
    for k in range(4):
        gU = gA[k] - gI[k]
        g.append(((-(gI[k] * a) + gU * b) - gU * cc) + gC[k] * d)
    box = (F64(2.0) - iou) - fill
    gd = [g[0] + g[2], g[1] + g[3], g[2] * pw if in2 else z, g[3] * ph if in3 else z]
    M = max(abs(float(v)) for v in (x0, y0, x1, y1, tx0, ty0, tx1, ty1))
    S = max(float(ew), float(eh))
    m = min(float(pw_), float(ph_), float(tx1 - tx0), float(ty1 - ty0))
    return box, gd, (M, S, m), dict(has=has, ties=(six0 and sex0, siy0 and sey0, six1 and sex1, siy1 and sey1), clamp=(not in2, not in3),
                                    inside=bool((six0 and siy0 and six1 and siy1) or (sex0 and sey0 and sex1 and sey1)))


def loss_ref(crout, crtarget, ccout, cctarget, npos, d, bgclass=None, roi=None, train=True):
    """-> dict: row_loss (R x 2 float64), key (R float32), box5 (with roi), cls, box (R float64), and under train crout (rows
    >= npos zeroed), crdelta, ccdelta (float32); err: dict of per-row fp64 error bounds (cls, box, gt: the target gradient, crdelta)
    -- all zero where the row involves no transcendental; info: per-row dicts of the GIoU selections."""
    crout = np.array(crout, F32).reshape(-1, 4)
    R = crout.shape[0]
    crtarget = np.asarray(crtarget, F32).reshape(R, 4)
    ccout = np.asarray(ccout, F32).reshape(R, -1)
    ncls = ccout.shape[1]
    cctarget = np.asarray(cctarget, F32).reshape(R)
    bgclass = ncls if bgclass is None else bgclass
    g, eps, beta, bw = F64(d["gamma"]), F64(d["label_smoothing"]), F64(d["beta"]), F64(d["box_weight"])
    focal = d["cls"] == "focal" and g > 0
    smooth = d["cls"] == "nll" and eps > 0
    cls = np.full(R, np.nan, F64); box = np.zeros(R, F64)
    ccdelta = np.zeros((R, ncls), F32); crdelta = np.zeros((R, 4), F32)
    key = np.zeros(R, F32)
    err = dict(cls=np.zeros(R), box=np.zeros(R), gt=np.zeros(R), crdelta=np.zeros((R, 4)))
    info = [None] * R
    Rd = F64(R)
    with np.errstate(all="ignore"):
        for r in range(R):
            tf = cctarget[r]
            valid = bool(tf >= F32(1.0) and tf <= F32(ncls))
            if valid:
                t = int(tf) - 1
                w = F64(1.0) if d["alpha"] is None else (F64(1.0) - F64(d["alpha"]) if t + 1 == bgclass else F64(d["alpha"]))
                lp = F64(ccout[r, t])
                if focal:
                    q = -np.expm1(lp)
                    if not q > 0.0:
                        q = F64(0.0)
                    qg = np.power(q, g)
                    cls[r] = -((w * qg) * lp)
                    x = ((g * np.power(q, g - F64(1.0))) * (F64(1.0) - q)) * lp if (q > 0.0 and lp > -np.inf) else F64(0.0)
                    ccdelta[r, t] = F32((w * (-qg + x)) / Rd)
                    if np.isfinite(cls[r]):
                        err["cls"][r] = (g * E1 + EP + 2 * ULP) * abs(cls[r])
                        err["gt"][r] = float(w / Rd) * ((g * E1 + EP + 4 * ULP) * qg + (abs(g - 1) * E1 + EP + 4 * ULP) * abs(x)
                                                         + g * E1 * qg * abs(lp))
                elif smooth:
                    u = eps / F64(ncls); ut = u + (F64(1.0) - eps)
                    s = F64(0.0)
                    for j in range(ncls):
                        s = s + (ut if j == t else u) * F64(ccout[r, j])
                    cls[r] = -(w * s)
                    ccdelta[r, :] = F32(-(w * u) / Rd)
                    ccdelta[r, t] = F32(-(w * ut) / Rd)
                else:
                    cls[r] = -(w * lp)
                    ccdelta[r, t] = F32(-w / Rd)
            fg = r < npos
            y = crout[r] if fg else np.zeros(4, F32)
            gd = [F64(0.0)] * 4
            if d["box"] == "smooth_l1":
                z = (y - crtarget[r]).astype(F32)
                terms = []
                for k in range(4):
                    zd = F64(z[k]); a = abs(zd)
                    quad = bool(a < beta)
                    terms.append(((F64(0.5) * zd) * zd) / beta if quad else a - F64(0.5) * beta)
                    gd[k] = zd / beta if quad else (F64(1.0) if zd > 0.0 else F64(-1.0))
                box[r] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
            elif fg:
                box[r], gd, (M, S, m), info[r] = giou_row(y, crtarget[r])
                if np.isfinite(box[r]) and m > 0:
                    e_s = 12 * ULP * (M + S)
                    err["box"][r] = 16 * S * e_s / m ** 2 + 6 * ULP
                    eg = float(bw) * 2 * max(1.0, S) * 4 * (2 / m ** 2 + 28 * S ** 2 / m ** 4) * e_s
                    err["crdelta"][r, :] = [eg + 8 * ULP * abs(float(bw * v)) for v in gd]
            crdelta[r] = [F32(bw * v) for v in gd]
            kv = F32(cls[r] + bw * box[r]) if valid else F32(-np.inf)
            key[r] = F32(np.inf) if np.isnan(kv) else kv
    out = dict(cls=cls, box=box, key=key, row_loss=np.stack([bw * box, cls / Rd], 1) if R else np.zeros((0, 2)), err=err, info=info)
    if roi is not None:
        out["box5"] = np.concatenate([np.asarray(roi, F64).reshape(R, 4).astype(F32), key[:, None]], 1)
    if train:
        cr = crout.copy(); cr[npos:] = 0.0
        out.update(crout=cr, crdelta=crdelta, ccdelta=ccdelta)
    return out


def accumulate_ref(row_loss):
    """frcnn_loss_accumulate's sum of R x 2 doubles in ITS order -> (sum of column 0, sum of column 1), and its stated bound
    R * 2^-53 * sum |terms| for each"""
    row_loss = np.asarray(row_loss, F64).reshape(-1, 2)
    out, bound = [], []
    with np.errstate(all="ignore"):
        for c in range(2):
            part = [F64(0.0)] * 64
            for e in range(row_loss.shape[0]):
                part[e % 64] = part[e % 64] + row_loss[e, c]
            o = 32
            while o > 0:
                for k in range(o):
                    part[k] = part[k] + part[k + o]
                o >>= 1
            out.append(float(part[0]))
            bound.append(row_loss.shape[0] * 2.0 ** -53 * float(np.abs(row_loss[:, c]).sum()))
    return tuple(out), tuple(bound)


# ------------------------------------------------------------------------------------------------------------------ the cases
SHAPES = [(1, 2, 0), (1, 3, 1), (63, 17, 1), (63, 3, 63), (63, 2, 0), (64, 21, 0), (64, 2, 64), (64, 17, 1), (65, 3, 1),
          (65, 17, 65), (65, 21, 0), (300, 21, 1), (300, 17, 300), (300, 3, 0)]          # (R, ncls, npos); R * ncls mod 4 != 0 at (1, 2), (1, 3), (63, 17), ...
DESCS = dict(
    default=desc(),
    beta_half=desc(beta=0.5, box_weight=1.0),
    beta_ninth=desc(beta=1.0 / 9.0, box_weight=3.0),
    smoothed=desc(label_smoothing=0.1),
    smoothed_alpha=desc(label_smoothing=0.25, alpha=0.75, box_weight=0.0),
    nll_alpha=desc(alpha=0.25),
    focal2=desc(cls="focal"),
    focal_half=desc(cls="focal", gamma=0.5, alpha=0.25),
    focal1_giou=desc(cls="focal", gamma=1.0, box="giou", box_weight=2.0),
    focal0=desc(cls="focal", gamma=0.0),
    giou=desc(box="giou"),
    giou_w0=desc(box="giou", box_weight=0.0),
)
EXACT = ("default", "beta_half", "beta_ninth", "smoothed", "smoothed_alpha", "nll_alpha", "focal0")   # no transcendental


def random_rows(seed, R, ncls, npos):
    """a table away from every tie: deltas of a net that is roughly right, log-probabilities of a LogSoftMax"""
    rng = np.random.RandomState(seed)
    crt = np.concatenate([rng.uniform(-0.6, 0.6, (R, 2)), rng.uniform(-0.7, 0.7, (R, 2))], 1).astype(F32)
    crt[npos:] = 0.0
    cro = (crt + rng.uniform(-0.45, 0.45, (R, 4)) + np.where(rng.rand(R, 4) < 0.2, rng.choice([-2.0, 2.0], (R, 4)), 0.0)).astype(F32)
    if npos < R:
        cro[npos:] = rng.randn(R - npos, 4).astype(F32)
    lg = rng.randn(R, ncls) * 2.0
    cco = (lg - np.log(np.exp(lg).sum(1, keepdims=True))).astype(F32)
    tgt = rng.randint(1, ncls + 1, R)
    tgt[npos:] = np.where(rng.rand(R - npos) < 0.7, ncls, tgt[npos:])
    roi = np.sort(rng.uniform(0, 400, (R, 4)).reshape(R, 2, 2), 1).reshape(R, 4)[:, [0, 2, 1, 3]].copy()
    return dict(crout=cro, crtarget=crt, ccout=cco, cctarget=tgt.astype(F32), roi=roi, R=R, ncls=ncls, npos=npos)


def _nx(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def edge_rows(c, d):
    """plants the labelled edge cases into a copy of the table c (rows permitting) -> (table, {label: [rows]}).  The labels are
    those of the issue's list; each is planted twice when the table has the rows for it."""
    c = dict((k, v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items())
    R, ncls, npos = c["R"], c["ncls"], c["npos"]
    lab = {}
    free = list(range(R))

    def take(fg=None):
        for i in free:
            if fg is None or (i < npos) == fg:
                free.remove(i)
                return i
        return None

    def plant(label, fn, fg=None, times=2):
        for n in range(times):
            r = take(fg)
            if r is None:
                return
            fn(r, n)
            lab.setdefault(label, []).append(r)

    def row_lsm(r, t, lp_t):          # a row whose target log-probability is lp_t exactly
        c["cctarget"][r] = t + 1
        c["ccout"][r, t] = lp_t

    plant("p_t_one", lambda r, n: row_lsm(r, n % ncls, 0.0))
    plant("neg_inf_target", lambda r, n: row_lsm(r, (n + 1) % ncls, -np.inf))

    def off(r, n):
        t = n % ncls
        c["cctarget"][r] = t + 1
        c["ccout"][r, (t + 1) % ncls] = -np.inf
    plant("neg_inf_off_target", off)
    plant("alpha_background", lambda r, n: c["cctarget"].__setitem__(r, ncls))
    if ncls > 1:
        plant("alpha_foreground", lambda r, n: c["cctarget"].__setitem__(r, 1 + n % (ncls - 1)))
    plant("bad_target", lambda r, n: c["cctarget"].__setitem__(r, [0.0, ncls + 1.0, np.nan, -3.0][n % 4]))

    def nan_row(r, n):
        t = n % ncls
        c["cctarget"][r] = t + 1
        c["ccout"][r, t] = np.nan
    plant("nan_input", nan_row)
    b32 = F32(d["beta"])

    def at_beta(r, n):       # |z| below, at (the float next to beta on either side of the double) and above beta, both signs
        c["crtarget"][r] = 0.0
        c["crout"][r] = [_nx(b32, False), b32, -_nx(b32, True), -b32] if n == 0 else [-_nx(b32, False), _nx(b32, True), b32 * 2, -b32 / 2]
    plant("z_at_beta", at_beta, fg=True)

    def boxes(pred, tgt):
        def fn(r, n):
            s = 0.5 * n                     # (the second planting: both boxes moved, the geometry kept)
            c["crout"][r] = [pred[0] + s, pred[1] - s, pred[2], pred[3]]
            c["crtarget"][r] = [tgt[0] + s, tgt[1] - s, tgt[2], tgt[3]]
        return fn
    plant("giou_disjoint", boxes([3.0, 0.25, 0.1, -0.2], [-2.0, 0.0, 0.3, 0.2]), fg=True)
    plant("giou_partial", boxes([0.5, 0.25, 0.1, -0.2], [0.0, 0.0, 0.3, 0.2]), fg=True)
    plant("giou_inside", boxes([0.25, 0.25, -1.5, -1.25], [0.0, 0.0, 0.5, 0.5]), fg=True)

    def equal(r, n):
        c["crout"][r] = c["crtarget"][r] = [0.125 * (n + 1), -0.25, 0.3 - n, -0.2]
    plant("giou_equal", equal, fg=True)
    plant("giou_edge_tie", boxes([0.5, 0.125, 0.4, -0.3], [0.5, 0.125, 0.1, 0.2]), fg=True)
    plant("giou_above_K", boxes([0.1, -0.1, 5.0, 4.5], [0.0, 0.0, 0.5, 0.25]), fg=True)
    return c, lab


LABELS = ("p_t_one", "neg_inf_target", "neg_inf_off_target", "alpha_background", "alpha_foreground", "bad_target", "nan_input",
          "z_at_beta", "giou_disjoint", "giou_partial", "giou_inside", "giou_equal", "giou_edge_tie", "giou_above_K")


def case(R, ncls, npos, name):
    d = DESCS[name]
    c, lab = edge_rows(random_rows(9000 + 131 * R + 7 * ncls + npos, R, ncls, npos), d)
    return c, lab, d
