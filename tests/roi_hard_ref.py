"""Restatement of frcnn_roi_hard_keys_batch and frcnn_roi_hard_gather_batch (include/frcnn_hip.h) for the tests: numpy, no GPU,
no library.

keys_ref: the per-row loss in np.float32, one rounded operation per statement, in the header's order:
    cls = -ccout[r][t-1];  foreground: z = crout - crtarget, a = |z|, term = a < 1 ? (0.5*z)*z : a - 0.5,
    reg = ((t0 + t1) + t2) + t3, reg = reg * 10;  background: reg = 0;  loss = cls + reg;  NaN -> +inf;  a target outside
    1 ... ncls -> -inf.
select_ref: the hard NMS of the library on {fp32 rect, loss} rows (soft_nms_ref's method hard with min_score = -inf: every row
    is alive, the largest key is picked, ties go to the higher row, a row dies when !(iou <= overlap)), then the gather's rule:
    the first `batch` picks within [1, n], leaving in ascending row order, foreground rows first.
gather_ref: the gather's rule alone, on any pick list."""
import math

import numpy as np

import soft_nms_ref as SN

F32 = np.float32
TABLE = (("roi", np.float64, 4), ("crtarget", np.float32, 4), ("cctarget", np.float32, 1), ("src", np.int32, 1), ("gt_idx", np.int32, 1),
         ("iou", np.float64, 1))


def keys_ref(roi, crout, crtarget, ccout, cctarget, nfg):
    """-> (box5 n x 5 fp32, loss n fp32)"""
    roi = np.asarray(roi, np.float64).reshape(-1, 4)
    n = roi.shape[0]
    crout = np.asarray(crout, np.float32).reshape(-1, 4)
    crtarget = np.asarray(crtarget, np.float32).reshape(-1, 4)
    ccout = np.asarray(ccout, np.float32)
    ncls = ccout.shape[1]
    cctarget = np.asarray(cctarget, np.float32).reshape(-1)
    loss = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            tf = cctarget[r]
            if not (tf >= F32(1.0) and tf <= F32(ncls)):
                loss[r] = -np.inf
                continue
            cls = F32(-ccout[r, int(tf) - 1])
            reg = F32(0.0)
            if r < nfg:
                term = []
                for k in range(4):
                    z = F32(crout[r, k] - crtarget[r, k])
                    a = F32(abs(z))
                    if a < F32(1.0):
                        h = F32(F32(0.5) * z)
                        term.append(F32(h * z))
                    else:
                        term.append(F32(a - F32(0.5)))
                reg = F32(term[0] + term[1])
                reg = F32(reg + term[2])
                reg = F32(reg + term[3])
                reg = F32(reg * F32(10.0))
            l = F32(cls + reg)
            loss[r] = np.inf if l != l else l
        box5 = np.concatenate([roi.astype(np.float32), loss[:, None]], axis=1)
    return box5, loss


def hard_nms(box5, overlap):
    """frcnn_nms_device_batch(key_mode 2, key_col 5) on one segment -> 1-based picks in pick order"""
    pick, _ = SN.soft_nms_f32(box5, 5, SN.HARD, overlap, 1.0, -math.inf, 0)
    return pick


def gather_ref(pick, count, batch, n, nfg, table, loss):
    """table: dict of the six "all" arrays (>= n rows) -> dict of the selected rows + loss, counts (F, Bq, count, n), rows: the
    selected 0-based rows in output order"""
    sel = []
    for p in list(pick)[:max(count, 0)]:
        if 1 <= p <= n:
            if len(sel) < batch:
                sel.append(int(p) - 1)
    rows = sorted(set(sel))
    F = sum(1 for i in rows if i < nfg)
    out = dict((name, np.asarray(table[name])[rows].copy()) for name, _, _ in TABLE)
    out["loss"] = np.asarray(loss, np.float32)[rows].copy()
    out["counts"] = (F, len(rows) - F, max(count, 0), n)
    out["rows"] = rows
    return out


def select_ref(box5, loss, nfg, batch, overlap, table):
    """keys -> NMS -> gather on one segment -> gather_ref's dict + pick (the survivors in pick order)"""
    n = len(loss)
    pick = hard_nms(box5, overlap) if n else np.zeros(0, np.int64)
    out = gather_ref(pick, len(pick), batch, n, nfg, table, loss)
    out["pick"] = pick
    return out


def iou_f32(b, i, j):
    """the NMS's fp32 IoU of rows i and j of box5 (+ 1 areas), as soft_nms_ref computes it"""
    f = np.float32
    x1, y1, x2, y2 = (b[:, k].astype(f) for k in range(4))
    with np.errstate(all="ignore"):
        area = lambda k: f(f(f(x2[k] - x1[k]) + f(1)) * f(f(y2[k] - y1[k]) + f(1)))
        w = f(f(min(x2[i], x2[j]) + f(f(-1) * max(x1[i], x1[j]))) + f(1))
        h = f(f(min(y2[i], y2[j]) + f(f(-1) * max(y1[i], y1[j]))) + f(1))
        w = w if w > 0 else f(0)
        h = h if h > 0 else f(0)
        inter = f(w * h)
        return f(inter / f(f(area(i) + area(j)) - inter))


# ---------------------------------------------------------------------------------------------------------------- cases
def random_table(rng, n, nfg, ncls, span=300.0, dup=0.0, equal_loss=0.0):
    """n labelled candidates: integer-cornered boxes in a span x span frame (`dup`: the share that copies an earlier box; `equal_loss`:
    the share whose net outputs copy an earlier row's, so that their losses tie when the labels agree), regression differences on
    both sides of 1, class targets valid, foreground rows first"""
    x = np.floor(rng.rand(n, 2) * span)
    wh = 8.0 + np.floor(rng.rand(n, 2) * span / 3)
    roi = np.concatenate([x, x + wh], axis=1).astype(np.float64)
    crtarget = (rng.randn(n, 4) * 0.7).astype(np.float32)
    crtarget[nfg:] = 0.0
    crout = (rng.randn(n, 4) * 0.9).astype(np.float32)
    logits = rng.randn(n, ncls) * 2.0
    ccout = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
    cctarget = (1 + rng.randint(0, max(ncls - 1, 1), n)).astype(np.float32)
    cctarget[nfg:] = float(ncls)
    for r in range(1, n):
        if rng.rand() < dup:
            roi[r] = roi[rng.randint(0, r)]
        if rng.rand() < equal_loss:
            q = rng.randint(nfg, r) if r > nfg else rng.randint(0, r)   # (background rows tie with background rows)
            crout[r], ccout[r] = crout[q], ccout[q]
            if (r < nfg) == (q < nfg):
                crtarget[r], cctarget[r] = crtarget[q], cctarget[q]
    return dict(roi=roi, crout=crout, crtarget=crtarget, ccout=ccout, cctarget=cctarget, nfg=nfg, ncls=ncls,
                src=(np.arange(n) + 3).astype(np.int32), gt_idx=np.where(np.arange(n) < nfg, np.arange(n) % 5, -1).astype(np.int32),
                iou=rng.rand(n).astype(np.float64))


def edge_rows(case):
    """plants the arithmetic edges in the first rows that exist: |z| exactly 1 and next to it on either side, a NaN and an inf in
    ccout and in crout, a target of 0 and of ncls + 1 (and a NaN target)"""
    c = dict((k, (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in case.items())
    n, nfg, ncls = len(c["cctarget"]), c["nfg"], c["ncls"]
    one = np.float32(1.0)
    zs = [one, -one, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), -np.nextafter(one, F32(0)), -np.nextafter(one, F32(2)),
          F32(0.0), F32(-0.0)]
    for r in range(min(nfg, 4)):
        c["crtarget"][r] = 0.0
        c["crout"][r] = [zs[(2 * r + k) % len(zs)] for k in range(4)]
    plant = [("crout", np.nan), ("crout", np.inf), ("crout", -np.inf)]
    for j, (name, v) in enumerate(plant):
        r = 4 + j
        if r < n:
            c[name][r, j % 4] = v
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        r = n - 1 - j
        if r >= 0:
            c["ccout"][r, int(c["cctarget"][r]) - 1] = v
    for j, v in enumerate((0.0, float(ncls + 1), np.nan, -3.0, 1e30)):
        r = n // 2 + j
        if 8 <= r < n - 3:
            c["cctarget"][r] = v
    return c


def table_of(case):
    return dict((name, case[name]) for name, _, _ in TABLE)
