"""Float64 restatement of RoIAlign as include/frcnn_hip.h states it (frcnn_roi_align_forward / _backward): plain loops, numpy
float64, no device code.  The geometry is written operation by operation as the header gives it, so a sample lands in the same
cell here and on the device unless it lies on one of the four discontinuities (near_discontinuities counts those).

  forward(fmap, rects, kh, kw, g, sx, sy, pick)            -> out (R, C*kh*kw), c-major rows like the max pool's
  backward(gout, rects, shape, kh, kw, g, sx, sy, pick,
           gmap0)                                          -> (gmap, count, abs_sum): gmap = gmap0 + scatter(gout); per element of
                                                              the map the number of terms of that sum and the sum of their
                                                              magnitudes.  gmap0 (the map the device adds into) is ONE term of
                                                              an element's sum when it is given: the device forms
                                                              gmap0 + t1 + ... + tn in fp32, so the worst-case bound of an fp32
                                                              sum of the n + 1 terms is the bar for it.  touched = count minus
                                                              that term.
  near_discontinuities(rects, H, W, kh, kw, g, sx, sy, pick, eps) -> samples within eps of y = -1, y = H, x = -1 or x = W

The statement divides by the stride; the kernels take 1 / S and multiply.  For a power-of-two stride (16 for both models, and
what every test here uses) the two are the same number, and only then does "the same cell" hold to the last bit.

rects: (n, 4) float64 {minX, minY, maxX, maxY} in input space; pick: optional 1-based rows of rects; sx, sy: the stride."""
import numpy as np


def _rows(rects, pick):
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    if pick is None:
        return rects
    return rects[np.asarray(pick, np.int64) - 1]


def _axis(v, n):
    """-> None (the sample contributes 0) or (lo, hi, l)"""
    if v < -1.0 or v > float(n):
        return None
    v = max(v, 0.0)
    lo = int(v)
    if lo >= n - 1:
        lo = hi = n - 1
        v = float(lo)
    else:
        hi = lo + 1
    return lo, hi, v - lo


def samples(rect, H, W, kh, kw, g, sx, sy):
    """Yields (i, j, y, x, taps) for the kh*kw*g*g samples of one rect, iy outer and ix inner within a bin; taps is None or the
    four ((yy, xx), weight) in the order (lo, lo), (lo, hi), (hi, lo), (hi, hi), the weights rounded to fp32 as on the device."""
    minX, minY, maxX, maxY = (np.float64(v) for v in rect)
    x1 = minX / sx - 0.5
    y1 = minY / sy - 0.5
    w = max((maxX - minX) / sx, 0.0)
    h = max((maxY - minY) / sy, 0.0)
    bin_w = w / kw
    bin_h = h / kh
    for i in range(kh):
        for j in range(kw):
            for iy in range(g):
                y = y1 + (i + (iy + 0.5) / g) * bin_h
                ay = _axis(y, H)
                for ix in range(g):
                    x = x1 + (j + (ix + 0.5) / g) * bin_w
                    ax = _axis(x, W)
                    if ay is None or ax is None:
                        yield i, j, y, x, None
                        continue
                    (ylo, yhi, ly), (xlo, xhi, lx) = ay, ax
                    hy, hx = 1.0 - ly, 1.0 - lx
                    wts = [np.float64(np.float32(v)) for v in (hy * hx, hy * lx, ly * hx, ly * lx)]
                    yield i, j, y, x, list(zip(((ylo, xlo), (ylo, xhi), (yhi, xlo), (yhi, xhi)), wts))


def forward(fmap, rects, kh, kw, g, sx=16.0, sy=16.0, pick=None):
    fmap = np.asarray(fmap, np.float64)
    C, H, W = fmap.shape
    rows = _rows(rects, pick)
    out = np.zeros((len(rows), C, kh, kw), np.float64)
    for r, rect in enumerate(rows):
        for i, j, _, _, taps in samples(rect, H, W, kh, kw, g, sx, sy):
            if taps is None:
                continue
            for (yy, xx), wt in taps:
                out[r, :, i, j] += wt * fmap[:, yy, xx]
    out /= float(g * g)
    return out.reshape(len(rows), C * kh * kw)


def backward(gout, rects, shape, kh, kw, g, sx=16.0, sy=16.0, pick=None, gmap0=None):
    C, H, W = shape
    rows = _rows(rects, pick)
    gout = np.asarray(gout, np.float64).reshape(len(rows), C, kh, kw)
    gmap = np.zeros(shape, np.float64)
    count = np.zeros(shape, np.int64)
    abs_sum = np.zeros(shape, np.float64)
    if gmap0 is not None:
        gmap += np.asarray(gmap0, np.float64)
        count += 1
        abs_sum += np.abs(np.asarray(gmap0, np.float64))
    inv = 1.0 / float(g * g)
    for r, rect in enumerate(rows):
        for i, j, _, _, taps in samples(rect, H, W, kh, kw, g, sx, sy):
            if taps is None:
                continue
            for (yy, xx), wt in taps:
                t = wt * gout[r, :, i, j] * inv
                nz = t != 0.0        # (a zero weight or a zero gradient adds nothing on the device either)
                gmap[:, yy, xx] += t
                count[:, yy, xx] += nz
                abs_sum[:, yy, xx] += np.abs(t)
    return gmap, count, abs_sum


def near_discontinuities(rects, H, W, kh, kw, g, sx=16.0, sy=16.0, pick=None, eps=1e-6):
    n = 0
    for rect in _rows(rects, pick):
        for _, _, y, x, _ in samples(rect, H, W, kh, kw, g, sx, sy):
            if min(abs(y + 1.0), abs(y - H), abs(x + 1.0), abs(x - W)) <= eps:
                n += 1
    return n
