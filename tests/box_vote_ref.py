"""Restatement of frcnn_box_vote_batch (include/frcnn_hip.h) for the tests: no GPU, no library.

  winners: the 1-based rows `picks`; for a winner row m, row j VOTES iff
      cls[j] == cls[m] (every row without cls)  and  iou(j, m) >= overlap (a NaN IoU is no vote)  and  w_j is finite and > 0
  w_j = 1 (weight_mode 0) | (double)score_j (1) | exp((double)score_j) (2)
  c_j = rect[j] (fp64) when rect is given, else (double)boxes[j][0..3]
  rect_out[m][t] = (sum w_j c_j[t]) / (sum w_j) over the voters; votes[m] = their number; fewer than two voters: c_m, bit for bit
  area = (x2-x1+1)*(y2-y1+1), w = max(0, (xx2 + (-1)*xx1) + 1), iou = (w*h) / ((area_j + area_m) - w*h)

MEMBERSHIP (and so `votes`) is numpy fp32, one rounded operation per statement -- the IoU statements are those of
soft_nms_ref._loop, in their order: the device must agree bit for bit.  (Under weight_mode 2 the weight test reads exp(score);
it is exact wherever exp neither underflows nor overflows in fp64, i.e. for every score in about (-700, 700).)

THE MEANS are computed EXACTLY from the fp64 inputs (the weights as this file's fp64 numbers, the coordinates as given) with
fractions.Fraction and rounded once to fp64.

rect_error_bound(k, A_t, weight_mode): the worst case of |device - restatement| for one coordinate of a winner with k >= 2
voters, A_t = (sum w_j |c_j[t]|) / (sum w_j).  With u = 2^-53, the unit roundoff of fp64:
  the device computes  fl( N^ / D^ ),  N^ = the floating-point sum, in SOME order, of the k rounded products fl(w_j c_j),
  D^ = the floating-point sum of the k weights in the same order.
  products      one rounding each:                                         fl(w_j c_j) = w_j c_j (1 + d),     |d| <= u
  numerator     a summand passes through at most k - 1 additions in any summation order (a chain, a tree, or the kernel's
                lanes-then-butterfly), each of which rounds once:          N^ = sum w_j c_j (1 + e_j),        |e_j| <= k u
                so |N^ - N| <= k u sum w_j |c_j|                                                             [+ O(u^2)]
  denominator   the same without the product:                             D^ = D (1 + z),                    |z| <= (k - 1) u
                (the weights are positive: the perturbed sum is D times a convex combination of the factors)
  quotient      N^/D^ - N/D = (N^ - N)/D^ + (N/D)(D/D^ - 1):               at most k u A_t + (k - 1) u |N/D|,  |N/D| <= A_t
  division      one rounding:                                              u |N^/D^| <= u A_t
  together (2 k) u A_t.
  weight_mode 2: the device's weight is exp() of the HIP math library, documented at 1 ULP (a relative 2 u at most); this
                file's is math.exp of the host libm, taken at 1 ULP as well: the two weights of a row differ by a relative
                e <= 4 u.  A mean whose weights move by relative e_j moves by  sum w_j e_j (c_j - M) / sum w_j (1 + e_j),
                at most e (A_t + |M|) <= 2 e A_t = 8 u A_t.  (weight_mode 0 and 1: both sides hold the same fp64 weights.)
  restatement   the exact rational rounded once to fp64:                   u A_t
  c(k) = 2 k + 1 (+ 8 under weight_mode 2), linear in k; the terms of second order are below k u times the first-order sum --
  below 2^-40 of it for any k a segment can hold -- and the bound is the first-order sum times (1 + 2^-10).
A winner with fewer than two voters has the bound 0."""
import math
from fractions import Fraction

import numpy as np

UNIFORM, SCORE, LOG_SCORE = 0, 1, 2
WEIGHTS = ("uniform", "score", "log_score")
U64 = 2.0 ** -53


def weights_f64(rows, score_col, weight_mode):
    """the n fp64 weights of the rows (math.exp under weight_mode 2: one libm call per row)"""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    if weight_mode == UNIFORM:
        return np.ones(n, np.float64)
    s = rows[:, score_col - 1].astype(np.float64)
    if weight_mode == SCORE:
        return s

    def ex(v):
        try:
            return math.exp(v)
        except OverflowError:
            return math.inf
    return np.array([ex(float(v)) for v in s], np.float64)


def membership_f32(rows, m, overlap, cls=None):
    """rows j with cls[j] == cls[m] and iou(j, m) >= overlap, as a boolean array: fp32, one rounded operation per statement
    (the statements of soft_nms_ref._loop)"""
    f = np.float32
    b = np.asarray(rows, np.float32)
    Nt = f(np.float32(overlap))
    one, zero = f(1), f(0)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(all="ignore"):
        dx = x2 - x1
        dy = y2 - y1
        dx = dx + one
        dy = dy + one
        area = dx * dy
        xx1 = np.where(x1 > x1[m], x1, x1[m])
        yy1 = np.where(y1 > y1[m], y1, y1[m])
        xx2 = np.where(x2 < x2[m], x2, x2[m])
        yy2 = np.where(y2 < y2[m], y2, y2[m])
        w = xx2 + f(-1) * xx1
        w = w + one
        w = np.where(w > zero, w, zero)
        h = yy2 + f(-1) * yy1
        h = h + one
        h = np.where(h > zero, h, zero)
        inter = w * h
        denom = area + area[m]
        denom = denom - inter
        iou = inter / denom
        member = iou >= Nt          # (a NaN compares false)
    if cls is not None:
        cls = np.asarray(cls)
        member = member & (cls == cls[m])
    return member


def box_vote(rows, picks, overlap, score_col=5, weight_mode=SCORE, cls=None, rect=None):
    """-> (rects: k x 4 float64, votes: k int32, A: k x 4 float64 -- A_t of every winner's coordinates, 0 where fewer than two
    rows voted), in the order of picks (1-based rows)"""
    rows = np.asarray(rows, np.float32)
    picks = np.asarray(picks, np.int64).reshape(-1)
    k = picks.size
    out, votes, A = np.zeros((k, 4), np.float64), np.zeros(k, np.int32), np.zeros((k, 4), np.float64)
    if k == 0:
        return out, votes, A
    wt = weights_f64(rows, score_col, weight_mode)
    ok = np.isfinite(wt) & (wt > 0)
    c = np.asarray(rect, np.float64) if rect is not None else rows[:, :4].astype(np.float64)
    for q, m in enumerate((picks - 1).tolist()):
        j = np.nonzero(membership_f32(rows, m, overlap, cls) & ok)[0]
        votes[q] = j.size
        if j.size < 2:
            out[q] = c[m]
            continue
        fw = [Fraction(float(v)) for v in wt[j]]
        D = sum(fw)
        for t in range(4):
            fc = [Fraction(float(v)) for v in c[j, t]]
            out[q, t] = float(sum(a * b for a, b in zip(fw, fc)) / D)
            A[q, t] = float(sum(a * abs(b) for a, b in zip(fw, fc)) / D)
    return out, votes, A


def rect_error_bound(k, A_t, weight_mode):
    """the worst case of |device - restatement| for one coordinate of a winner with k voters (derivation: the module's docstring)"""
    if k < 2:
        return 0.0
    c = 2.0 * k + 1.0 + (8.0 if weight_mode == LOG_SCORE else 0.0)
    return c * U64 * float(A_t) * (1.0 + 2.0 ** -10)
