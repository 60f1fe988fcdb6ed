"""The native model at widths between the narrow parity variants and the reference ones (tests/width_plan.py: the tables
and the branch each entry exists to reach), against the oracle with the device's decisions injected (SURVEY 8d's bars),
and the sparse anchor nets against the dense convolutions at the position counts where their planner changes."""
import ctypes as C

import numpy as np
import pytest

import decisions
import width_plan as WP
from test_gpu_model import _OneBatch, _compare_gradient, _masks, check_loss_and_gradient, check_pnet_forward_backward
from util import assert_close

pytestmark = pytest.mark.gpu


def _build(F, O, filters, heads, cls, seed=11):
    cfg = dict(F.duplo_cfg)
    layers, anchor_nets, class_layers = WP.layers_of(filters), WP.heads_of(heads), WP.cls_of(*cls)
    assert len(anchor_nets) == len(cfg["scales"])
    model = F.create_model(cfg, layers, anchor_nets, class_layers)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=seed)
    om = O.make_model(layers, anchor_nets, class_layers, cfg)
    assert O.param_count(om) == (model["native"].total_params, model["native"].pnet_params)
    return dict(cfg=cfg, model=model, weights=weights, gradient=gradient, om=om, w=weights.cpu().numpy().copy())


def _examples(F, model, cfg, H, W, positions, seed):
    """One image whose examples lie at exactly positions[l] distinct (y, x) of anchor net l (Anchors.get, as
    test_gpu_golden_e2e.py builds them): one aspect per position, a second one at every fifth position (the aspects of one
    position are one position of the sparse path), every fourth example a positive with a ROI of its own (a ROI pooling
    window shared by many rows would count each of its cell winners that many times in the decision statistics)."""
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    sizes = F.output_map_sizes(model, H, W)
    rng = np.random.RandomState(seed)
    rois = F.synthetic_rois(cfg, W, H, sum(WP.cdiv(P, 4) for P in positions), 7, seed)
    pos, neg = [], []
    for l, P in enumerate(positions):
        h, w = sizes[l]
        assert P <= h * w, (l, P, h, w)
        for j, p in enumerate(rng.choice(h * w, P, replace=False)):
            a = anchors.get(l + 1, j % 3 + 1, int(p) // w + 1, int(p) % w + 1)
            if j % 4 == 0:
                pos.append((a, rois[len(pos)]))
            else:
                neg.append((a,))
            if j % 5 == 0:
                neg.append((anchors.get(l + 1, (j + 1) % 3 + 1, int(p) // w + 1, int(p) % w + 1),))
    assert F.clean_examples(pos, sizes) == pos and F.clean_examples(neg, sizes) == neg
    for l, P in enumerate(positions):   # the count the sparse path sees (objective.py prepare_examples)
        got = {(e[0].index[1], e[0].index[2]) for e in pos + neg if e[0].layer == l + 1}
        assert len(got) == P
    return F.synthetic_image(H, W, seed), rois, pos, neg


# ---- part 1: the configurations against the oracle ---------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(WP.CONFIGS))
def config(request, F, O):
    c = WP.CONFIGS[request.param]
    return request.param, c, _build(F, O, c["filters"], c["heads"], c["cls"])


def test_pnet_forward_backward(F, O, config):
    name, c, s = config
    rng = np.random.RandomState(0)
    H, W = WP.SMALL
    img = F.synthetic_image(H, W, 0)
    check_pnet_forward_backward(F, O, s, img, _masks(rng, s["model"]), rng, what=name)


def test_loss_and_gradient(F, O, config):
    name, c, s = config
    H, W = c["frame"]
    ex = _examples(F, s["model"], s["cfg"], H, W, c["positions"], seed=2)
    # the ROI pooling windows of every example (anchors that reach beyond the frame included) are the oracle's: the
    # injected cell winners below cannot hide a window that differs
    img, rois, pos, neg = ex
    rects = np.array([[r.rect.minX, r.rect.minY, r.rect.maxX, r.rect.maxY] for a, r in pos] +
                     [[e[0].minX, e[0].minY, e[0].maxX, e[0].maxY] for e in neg], dtype=np.float64)
    fh, fw = H, W
    for _ in c["filters"]:
        fh, fw = -(-(fh - 2) // 2) + 1, -(-(fw - 2) // 2) + 1
    loc = F.Localizer(s["model"]["pnet"].outnode.children[len(c["heads"])])
    layers = O.model_localizer_layers(s["om"], len(c["heads"]) + 1)
    want = np.array([O.extract_roi_window(layers, r, fh, fw) for r in rects], dtype=np.int32)
    assert np.array_equal(F.roi_windows(rects, loc, fh, fw), want)
    check_loss_and_gradient(F, O, s, H, W, examples=[ex])


@pytest.fixture(scope="module", params=WP.CNET_CONFIGS)
def cnet_config(request, F, O):
    c = WP.CONFIGS[request.param]
    return request.param, c, _build(F, O, c["filters"], c["heads"], c["cls"])


@pytest.mark.parametrize("R", WP.CNET_ROWS)
def test_cnet_rows(F, O, cnet_config, R):
    """cnet forward / backward against the oracle at row counts on either side of linear_x_eligible's R >= 32 and >= 192,
    on classification widths the split product takes (2304) and does not take (1000, 500)."""
    name, c, s = cnet_config
    rng = np.random.RandomState(R)
    n1, n2 = c["cls"]
    D = WP.ROI_CELLS * c["filters"][-1]
    ncls = s["cfg"]["class_count"] + 1
    x = rng.randn(R, D).astype(np.float32)
    cmasks = [(rng.rand(R, n1) > 0.5).astype(np.float32), (rng.rand(R, n2) > 0.5).astype(np.float32)]
    cnet, native = s["model"]["cnet"], s["model"]["native"]
    bn0 = native.bn_running.cpu().numpy().copy()
    cnet.training()
    cnet.drop_masks = cmasks
    try:
        bbox, cls = cnet.forward(x)
        # the device's PReLU branches injected into the oracle (tests/decisions.py): R x 2304 of them, a pre-activation within
        # rounding of 0 is no rarity, and one branch taken differently moves a whole row of the weight gradient
        dec = dict(cnet_pos=[np.ascontiguousarray((decisions._dev_array(F, native, 3, i, np.float32, (R, n)) > 0).astype(np.uint8))
                             for i, n in enumerate((n1, n2))])
        own = decisions.blank_like(dec)
        bn_o = bn0.copy()
        g_want = np.zeros_like(s["w"])
        gb = rng.randn(R, 4).astype(np.float32); gc = (rng.randn(R, ncls) / R).astype(np.float32)
        with O.decisions(inject=dec, record=own):
            wb, wc, st = O.cnet_forward(s["om"], s["w"], x, True, cmasks, bn_o)
            gx_want = O.cnet_backward(s["om"], s["w"], st, gb, gc, g_want, D)
        assert_close(bbox.numpy(), wb, 1e-4, "cnet bbox")
        assert_close(cls.numpy(), wc, 1e-4, "cnet cls")
        assert_close(native.bn_running.cpu().numpy(), bn_o, 1e-5, "bn running stats")
        nd, nt = decisions.count_differences(dec, own)["cnet_pos"]
        assert nd <= max(4, 2e-5 * nt), (nd, nt)
        s["gradient"].zero_()
        gx = cnet.backward(x, [F.DeviceTensor.from_numpy(gb), F.DeviceTensor.from_numpy(gc)])
        assert_close(gx.numpy(), gx_want, 1e-4, "cnet gradInput")
        _compare_gradient(native, s["gradient"].cpu().numpy(), g_want, lo=native.pnet_params, hi=native.total_params)
    finally:
        cnet.drop_masks = None
        import torch
        native.bn_running.copy_(torch.from_numpy(bn0))


# ---- part 2: sparse anchor nets against the dense convolutions, position sweep -----------------------------------------
def _step(F, s, ex, sparse, seed):
    import torch
    model = s["model"]
    img, rois, pos, neg = ex
    anchors = F.Anchors(model["pnet"], s["cfg"]["scales"])
    rng = np.random.RandomState(seed)
    E = len(pos) + len(neg)
    F._lib.call("frcnn_set_option", b"sparse_heads", 1 if sparse else 0)
    try:
        model["pnet"].drop_masks = _masks(rng, model)
        model["cnet"].drop_masks = [(rng.rand(E, l["n"]) > 0.5).astype(np.float32) for l in model["class_layers"]]
        f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch([dict(img=img, positive=pos, negative=neg)], anchors),
                               dict(pcls=[], preg=[], dcls=[], dreg=[]))
        loss, grad = f(s["weights"])
        torch.cuda.synchronize()
        return loss, grad.cpu().numpy().copy()
    finally:
        F._lib.call("frcnn_set_option", b"sparse_heads", 1)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None


@pytest.mark.parametrize("n", WP.SWEEP_WIDTHS)
def test_sparse_anchor_nets_position_sweep(F, O, n):
    """P distinct positions on each of the four n-wide anchor nets: loss within 1e-6, every gradient tensor within 2e-5 L2
    of the dense convolutions (as test_gpu_sparse_heads.py; a PReLU slope, one number, within 1e-3), the K-split planner
    of heads_jobs at every P."""
    import torch
    s = _build(F, O, WP.VGG_BACKBONE, WP.vgg_heads(n), (1024, 512))
    nat = s["model"]["native"]
    lo, hi = s["model"]["pnet"].heads_param_range()
    bn0 = nat.bn_running.cpu().numpy().copy()
    H, W = WP.SWEEP_FRAME
    for P in WP.SWEEP_POSITIONS:
        ex = _examples(F, s["model"], s["cfg"], H, W, (P,) * WP.SCALES, seed=P)
        la, ga = _step(F, s, ex, True, P)
        nat.bn_running.copy_(torch.from_numpy(bn0))
        lb, gb = _step(F, s, ex, False, P)
        nat.bn_running.copy_(torch.from_numpy(bn0))
        assert np.isfinite(la) and abs(la - lb) <= 1e-6 * abs(lb), (n, P, la, lb)
        for off, cnt, kind, aux in nat.param_table:
            a, b = ga[off:off + cnt].astype(np.float64), gb[off:off + cnt].astype(np.float64)
            if np.linalg.norm(b) < 1e-4:
                continue
            # A PReLU slope's gradient is ONE sum over a whole layer of terms x * gy of either sign (test_gpu_model.py
            # _compare_gradient): the rounding of the terms, which is all the two ways differ in, is relative to their
            # absolute sum, which with a handful of sampled positions can be a thousand times the result (up to 8e-5 seen)
            bar = 1e-3 if kind == 2 else 2e-5
            assert np.linalg.norm(a - b) <= bar * np.linalg.norm(b), (n, P, off, cnt, kind, np.linalg.norm(a - b) / np.linalg.norm(b))
        assert np.abs(ga[lo:hi]).max() > 0


@pytest.mark.parametrize("n", WP.ORACLE_WIDTHS)
def test_anchor_net_width_against_the_oracle(F, O, n):
    """vgg_small's backbone with n-wide anchor nets, the whole objective against the oracle at vgg_small_n128's frame and
    positions (more than the K-split slab held before the cap for every n < 256)."""
    c = WP.CONFIGS["vgg_small_n128"]
    s = _build(F, O, WP.VGG_BACKBONE, WP.vgg_heads(n), c["cls"])
    H, W = c["frame"]
    ex = _examples(F, s["model"], s["cfg"], H, W, c["positions"], seed=2)
    check_loss_and_gradient(F, O, s, H, W, examples=[ex])


# ---- part 3: drop-compact boundaries against the oracle ----------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(WP.COMPACT_CONFIGS))
def compact_config(request, F, O):
    c = WP.COMPACT_CONFIGS[request.param]
    return request.param, c, _build(F, O, c["filters"], c["heads"], c["cls"])


@pytest.mark.parametrize("kept", WP.COMPACT_KEPT)
def test_compact_boundaries(F, O, compact_config, kept):
    """Explicit keep vectors with `kept` of C filters kept on every dropout block (C - 16: the last count that runs compact;
    C - 15 and C: nkK >= C, the block runs dense): the objective against the oracle, and the keep vector the device used
    (debug buffer kind 4) is the one passed in."""
    name, c, s = compact_config
    model, nat = s["model"], s["model"]["native"]
    rng = np.random.RandomState(5)
    pm = []
    for l in model["layers"]:
        if l["dropout"] <= 0:
            pm.append(None)
            continue
        keep = np.zeros(l["filters"], np.float32)
        keep[rng.choice(l["filters"], WP.kept_count(kept, l["filters"]), replace=False)] = 1.0
        pm.append(keep)
    H, W = c["frame"]
    ex = _examples(F, model, s["cfg"], H, W, c["positions"], seed=3)
    check_loss_and_gradient(F, O, s, H, W, examples=[ex], pmasks=pm)
    for b, keep in enumerate(pm):
        if keep is None:
            continue
        p = C.c_void_p(); nb = C.c_longlong()
        F._lib.call("frcnn_model_debug_buffer", nat.h, 4, b, C.byref(p), C.byref(nb))
        got = F.DeviceTensor(p.value, keep.shape, np.float32).numpy()
        assert np.array_equal(got, keep), "block %d: the device's keep vector is not the one passed in" % b
