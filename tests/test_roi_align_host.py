"""RoIAlign on the host: the setting (roi_pooling_settings), the stride and centredness of the backbones (Localizer), and the
float64 reference of tests/roi_align_ref.py against facts that do not depend on it."""
import numpy as np
import pytest

import roi_align_ref as ref


def _cfg(F, table):
    cfg = dict(F.duplo_cfg)
    cfg["roi_pooling"] = table
    return cfg


def test_settings_defaults_and_values(F):
    S = lambda table: F.roi_pooling_settings(_cfg(F, table))
    assert F.roi_pooling_settings(dict(F.duplo_cfg)) == (6, 6, "max", 2)
    assert S(dict(kw=6, kh=6)) == (6, 6, "max", 2)
    assert S(dict(kw=7, kh=5, method="max")) == (5, 7, "max", 2)
    assert S(dict(kw=7, kh=5, method="align")) == (5, 7, "align", 2)
    for g in (1, 2, 3, 4, np.int32(3)):
        got = S(dict(kw=6, kh=6, method="align", sampling_ratio=g))
        assert got == (6, 6, "align", int(g)) and type(got[3]) is int
    assert S(dict(kw=6, kh=6, method="max", sampling_ratio=99)) == (6, 6, "max", 2)   # only read under "align"


@pytest.mark.parametrize("table", [
    dict(kw=6, kh=6, mode="align"),                              # unknown key
    dict(kw=6, kh=6, method="avg"),                              # unknown method
    dict(kw=6, kh=6, method=1),
    dict(kw=6, kh=6, method="align", sampling_ratio=True),       # a bool
    dict(kw=6, kh=6, method="align", sampling_ratio=2.0),        # not an integer
    dict(kw=6, kh=6, method="align", sampling_ratio="2"),
    dict(kw=6, kh=6, method="align", sampling_ratio=None),
    dict(kw=6, kh=6, method="align", sampling_ratio=0),          # out of range
    dict(kw=6, kh=6, method="align", sampling_ratio=5),
    dict(kw=6, kh=6, method="align", sampling_ratio=-1),
])
def test_settings_reject(F, table):
    with pytest.raises(ValueError):
        F.roi_pooling_settings(_cfg(F, table))


@pytest.mark.parametrize("name", ["vgg_small", "vgg_large"])
def test_stride_and_centred(F, name):
    cfg = dict(F.duplo_cfg if name == "vgg_small" else F.imgnet_cfg)
    model = getattr(F, name)(cfg)
    loc = F.Localizer(model["pnet"].outnode.children[-1])
    assert loc.stride() == (16, 16)
    assert loc.centred()
    # an anchor net's path ends in a valid k x k convolution: not centred
    assert not F.Localizer(model["pnet"].outnode.children[0]).centred()
    assert F.Localizer([(3, 3, 1, 1, 1, 1), (2, 2, 2, 2, 0, 0), (2, 3, 2, 3, 0, 0)]).stride() == (4, 6)
    assert not F.Localizer([(3, 3, 1, 1, 0, 0)]).centred()
    assert not F.Localizer([(3, 3, 1, 1, 1, 0)]).centred()


def _inner_rects(rng, n, H, W, kh, kw, g, s):
    """rects whose samples all lie in [0, H-1] x [0, W-1] (feature coordinates), drawn from a continuous distribution"""
    out = []
    while len(out) < n:
        x0, x1 = np.sort(rng.uniform(0.5, W - 0.5, 2)); y0, y1 = np.sort(rng.uniform(0.5, H - 0.5, 2))
        rect = np.array([x0 * s, y0 * s, x1 * s, y1 * s])
        ok = all(0.0 <= y <= H - 1 and 0.0 <= x <= W - 1 for _, _, y, x, _ in ref.samples(rect, H, W, kh, kw, g, s, s))
        if ok:
            out.append(rect)
    return np.array(out)


@pytest.mark.parametrize("kh,kw,g", [(6, 6, 2), (2, 3, 3), (1, 1, 1), (7, 7, 4)])
def test_reference_on_constant_and_ramp(kh, kw, g):
    rng = np.random.RandomState(kh * 100 + kw * 10 + g)
    C, H, W, s = 3, 9, 13, 16.0
    rects = _inner_rects(rng, 6, H, W, kh, kw, g, s)
    const = np.full((C, H, W), 2.75)
    out = ref.forward(const, rects, kh, kw, g, s, s)
    assert np.abs(out - 2.75).max() <= 1e-6            # (the weights are rounded to fp32: four of them sum to 1 within 2^-22)
    a, b = 0.37, -1.21
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ramp = np.broadcast_to(a * yy + b * xx, (C, H, W))
    out = ref.forward(ramp, rects, kh, kw, g, s, s).reshape(len(rects), C, kh, kw)
    # without the fp32 rounding of the weights the reference is exact on a ramp: restate it with exact weights through the
    # samples it generates, and compare with the ramp at each bin's centre to 1e-12
    for r, rect in enumerate(rects):
        x1 = rect[0] / s - 0.5; y1 = rect[1] / s - 0.5
        bw = (rect[2] - rect[0]) / s / kw; bh = (rect[3] - rect[1]) / s / kh
        acc = np.zeros((kh, kw))
        for i, j, y, x, taps in ref.samples(rect, H, W, kh, kw, g, s, s):
            (ylo, xlo), (yhi, xhi) = taps[0][0], taps[3][0]
            ly, lx = y - ylo, x - xlo
            v = ((1 - ly) * (1 - lx) * ramp[0, ylo, xlo] + (1 - ly) * lx * ramp[0, ylo, xhi]
                 + ly * (1 - lx) * ramp[0, yhi, xlo] + ly * lx * ramp[0, yhi, xhi])
            acc[i, j] += v / (g * g)
        for i in range(kh):
            for j in range(kw):
                centre = a * (y1 + (i + 0.5) * bh) + b * (x1 + (j + 0.5) * bw)
                assert abs(acc[i, j] - centre) <= 1e-12 * max(1.0, abs(centre)), (r, i, j)
                # the reference itself: the same up to the fp32 rounding of its weights (4 g^2 weights of 2^-24 relative)
                assert abs(out[r, 0, i, j] - centre) <= 4 * 2.0 ** -24 * (abs(a) * H + abs(b) * W), (r, i, j)


def test_reference_ramp_exact_weights_cell_centres():
    """rects cut on whole cells with g = 1: every sample sits on a cell centre... of a bin one cell wide, the weights are
    exactly representable (0 or 1), and the reference equals the ramp at the bin's centre to 1e-12"""
    C, H, W, s, kh, kw = 2, 8, 10, 16.0, 3, 4
    a, b = 1.5, -0.25
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ramp = np.broadcast_to(a * yy + b * xx, (C, H, W))
    rect = np.array([[2 * s, 1 * s, (2 + kw) * s, (1 + kh) * s]])     # bins one cell wide, starting on a cell edge
    out = ref.forward(ramp, rect, kh, kw, 1, s, s).reshape(C, kh, kw)
    for i in range(kh):
        for j in range(kw):
            centre = a * (1 - 0.5 + i + 0.5) + b * (2 - 0.5 + j + 0.5)
            assert abs(out[0, i, j] - centre) <= 1e-12
    # ... and half-cell weights (0.5, exactly representable) with g = 2
    out = ref.forward(ramp, rect, kh, kw, 2, s, s).reshape(C, kh, kw)
    for i in range(kh):
        for j in range(kw):
            centre = a * (1 - 0.5 + i + 0.5) + b * (2 - 0.5 + j + 0.5)
            assert abs(out[0, i, j] - centre) <= 1e-12


@pytest.mark.parametrize("kh,kw,g", [(6, 6, 2), (2, 3, 3), (1, 1, 1)])
def test_reference_adjoint(kh, kw, g):
    rng = np.random.RandomState(7 + g)
    C, H, W, s = 3, 5, 7, 16.0
    rects = np.stack([rng.uniform(-40, 60, 12), rng.uniform(-40, 40, 12), rng.uniform(20, 160, 12), rng.uniform(10, 120, 12)], 1)
    pick = np.array([3, 12, 1, 7, 7], np.int64)
    x = rng.randn(C, H, W)
    gout = rng.randn(len(pick), C * kh * kw)
    lhs = float(np.sum(ref.forward(x, rects, kh, kw, g, s, s, pick) * gout))
    gm, count, abs_sum = ref.backward(gout, rects, (C, H, W), kh, kw, g, s, s, pick)
    rhs = float(np.sum(x * gm))
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), 1e-30)
    assert np.all((count == 0) == (abs_sum == 0)) and np.all(np.abs(gm) <= abs_sum * (1 + 1e-12))


def test_reference_outside_and_degenerate():
    C, H, W, s = 2, 4, 6, 16.0
    x = np.random.RandomState(0).randn(C, H, W)
    far = np.array([[-400.0, -300.0, -200.0, -100.0]])
    assert not np.any(ref.forward(x, far, 2, 2, 2, s, s))
    gm, count, _ = ref.backward(np.ones((1, C * 4)), far, (C, H, W), 2, 2, 2, s, s)
    assert not np.any(gm) and not np.any(count)
    # zero width and height at a cell centre: every sample is that cell
    point = np.array([[2.5 * s, 1.5 * s, 2.5 * s, 1.5 * s]])
    out = ref.forward(x, point, 2, 3, 2, s, s).reshape(C, 2, 3)
    assert np.allclose(out, x[:, 1, 2][:, None, None], rtol=0, atol=1e-15)
    assert ref.near_discontinuities(np.array([[-0.5 * s, 0, 3 * s, 2 * s]]), H, W, 1, 1, 1, s, s) == 0
    assert ref.near_discontinuities(np.array([[-0.5 * s, 0, -0.5 * s, 2 * s]]), H, W, 1, 1, 1, s, s) == 1   # x = -1 exactly
