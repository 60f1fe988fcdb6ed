"""cfg["box_head"] = {per_class = true} in the model, the training step, the optimisers and the Detector.  Tiny nets on 128 x 176
frames (vgg_small only where the Detector's fixtures need it).
  * class_layers = []: the head reads the pooled rows, so forward, backward's gx and the head's slice of the flat gradient are the
    op's entry points on the same arrays, bit for bit, for the three class sources; everything outside the box head's slice is
    the shared-head model's, bit for bit;
  * class_count = 1, where both layouts coincide: a per-class and a shared model on the same flat weights run one step;
  * key absent against {per_class = false}: bit-equal weights after two steps;
  * the Detector with zero box-head weights and one bias per class: exact against a shared-head model per class;
  * optimisers and staged training on the longer vector."""
import ctypes as C

import numpy as np
import pytest

import box_head_ref as B
import cnet_plan as CP
import width_plan as WP
from test_gpu_detect_batch import _amplified_weights, _frames, _winner_rows
from test_gpu_optim import _host, same_bits

pytestmark = pytest.mark.gpu

H, W = 128, 176
PER = dict(per_class=True)


def tiny(F, cc, box_head=None, cls_layers=(), L=16, seed=11, weights_host=None):
    cfg = dict(F.duplo_cfg, class_count=cc)
    if box_head is not None:
        cfg["box_head"] = dict(box_head)
    model = F.create_model(cfg, WP.layers_of(CP.BACKBONE + [L]), WP.heads_of(CP.HEADS), [dict(l) for l in cls_layers])
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=seed, weights_host=weights_host)
    return model, w, g


def head(nat):
    """-> (offset of the box head's weight, of its bias, the end of the block, nf, rows)"""
    (ow, nw, kw, nf), (ob, nb, kb, _) = (tuple(int(v) for v in r) for r in nat.param_table[-4:-2])
    assert (kw, kb) == (3, 4) and nw == nb * nf and ob == ow + nw
    return ow, ob, ob + nb, nf, nb


def shared_weights(nat_per, w_per, c):
    """the flat vector of the shared-head twin of a per-class model: the box head is class c's four rows, the rest as it is"""
    ow, ob, end, nf, rows = head(nat_per)
    return np.concatenate([w_per[:ow], w_per[ow + 4 * (c - 1) * nf:ow + 4 * c * nf], w_per[ob + 4 * (c - 1):ob + 4 * c], w_per[end:]])


def dptr(t, off_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * off_floats)


# ---- 1. class_layers = []: the model's passes are the op's entry points ---------------------------------------------------------
@pytest.mark.parametrize("source", ["int", "float", "none"])
def test_model_passes_equal_the_entry_points(F, source):
    cc, R = 5, 37
    model, w, g = tiny(F, cc, PER)
    nat, cnet = model["native"], model["cnet"]
    ow, ob, end, nf, rows = head(nat)
    assert rows == 4 * cc and nf == 36 * 16 and not nat.desc.ncls
    rng = np.random.RandomState(3)
    x = F.DeviceTensor.from_numpy(rng.standard_normal((R, nf)).astype(np.float32))
    cl_i = F.DeviceTensor.from_numpy(rng.randint(1, cc + 1, R).astype(np.int32))
    cl_f = F.DeviceTensor.from_numpy(rng.randint(1, cc + 2, R).astype(np.float32))       # (the background among them)
    n_fg = 20
    box_classes = {"int": ("int", cl_i, n_fg), "float": ("float", cl_f), "none": None}[source]
    bbox, cls = cnet.forward(x, box_classes=box_classes)
    bbox_h, cls_h = bbox.numpy().copy(), cls.numpy().copy()
    # the op on the same arrays (the class source "none" reads the pass's own log-probabilities)
    out, sel = F.DeviceTensor.zeros((R, 4)), F.DeviceTensor.zeros((R,), np.int32)
    kind, cp, n = {"int": (1, F.ptr(cl_i), n_fg), "float": (2, F.ptr(cl_f), 0), "none": (0, None, 0)}[source]
    s = F.stream_ptr()
    F._lib.call("frcnn_box_head_forward", F.ptr(x), R, nf, dptr(w, ow), dptr(w, ob), cc, cp, kind, n, F.ptr(cls), cc + 1,
                F.ptr(out), F.ptr(sel), s)
    sel_h = sel.numpy().copy()
    want = B.select(R, cc, {"int": "int", "float": "float", "none": "argmax"}[source],
                    {"int": cl_i, "float": cl_f, "none": None}[source].numpy() if source != "none" else None, n_fg, cls_h)
    assert np.array_equal(sel_h, want) and (sel_h > 0).sum() >= 10
    assert same_bits(bbox_h, out.numpy()) and bbox_h[sel_h > 0].any() and not bbox_h[sel_h == 0].any()
    # backward with a zero class gradient: gx is the box head's input gradient alone
    gb = F.DeviceTensor.from_numpy(rng.standard_normal((R, 4)).astype(np.float32))
    gc0 = F.DeviceTensor.zeros((R, cc + 1))
    g.zero_()
    gx = cnet.backward(x, [gb, gc0])
    gx_h = gx.numpy().copy()
    cnet.join_backward()
    g_h = _host(g).copy()
    gfeat, gW, gbias = F.DeviceTensor.zeros((R, nf)), F.DeviceTensor.zeros((rows, nf)), F.DeviceTensor.zeros((rows,))
    F._lib.call("frcnn_box_head_backward", F.ptr(gb), F.ptr(x), F.ptr(sel), R, nf, dptr(w, ow), cc, F.ptr(gfeat), F.ptr(gW),
                F.ptr(gbias), s)
    assert np.array_equal(gx_h, gfeat.numpy()) and gx_h.any()          # (== : the class head adds +0 to a -0)
    assert same_bits(g_h[ow:ob], gW.numpy().ravel()) and same_bits(g_h[ob:end], gbias.numpy()) and g_h[ow:ob].any()
    absent = np.repeat(np.bincount(sel_h, minlength=cc + 1)[1:] == 0, 4)
    assert not g_h[ow:ob].reshape(rows, nf)[absent].any()
    assert not g_h[:ow].any() and not g_h[end:].any()                  # zero class gradient: nothing else moves
    # the class source served that pass only: the next one predicts
    bbox2, cls2 = cnet.forward(x)
    F._lib.call("frcnn_box_head_forward", F.ptr(x), R, nf, dptr(w, ow), dptr(w, ob), cc, None, 0, 0, F.ptr(cls2), cc + 1,
                F.ptr(out), F.ptr(sel), s)
    assert same_bits(bbox2.numpy(), out.numpy())


@pytest.mark.parametrize("layers", [(), (dict(n=32, dropout=0.0),)], ids=["no_hidden_layer", "one_hidden_layer"])
def test_everything_outside_the_box_head_is_the_shared_model(F, monkeypatch, layers):
    """a zero box gradient (the box head then sends nothing down, in either model), separate launches in both models: the class
    head's slice, the hidden layer's and gx are the shared-head model's, bit for bit, at offsets moved by 4 (C - 1) (nf + 1)"""
    monkeypatch.setenv("FRCNN_CNET_FUSE", "0")
    cc, R = 5, 37
    mp, wp, gp = tiny(F, cc, PER, layers)
    ow, ob, end, nf, rows = head(mp["native"])
    ms, ws, gs = tiny(F, cc, None, layers, weights_host=shared_weights(mp["native"], _host(wp), 3))
    sow, sob, send, snf, srows = head(ms["native"])
    grow = 4 * (cc - 1) * (nf + 1)
    assert (sow, snf, srows) == (ow, nf, 4) and mp["native"].total_params == ms["native"].total_params + grow
    rng = np.random.RandomState(4)
    D = 36 * 16
    x = F.DeviceTensor.from_numpy(rng.standard_normal((R, D)).astype(np.float32))
    cl_f = F.DeviceTensor.from_numpy(rng.randint(1, cc + 2, R).astype(np.float32))
    gb0 = F.DeviceTensor.zeros((R, 4))
    gc = F.DeviceTensor.from_numpy(rng.standard_normal((R, cc + 1)).astype(np.float32))
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        res = []
        for model, g, bc in ((mp, gp, ("float", cl_f)), (ms, gs, None)):
            bbox, cls = model["cnet"].forward(x, box_classes=bc)
            cls_h = cls.numpy().copy()
            g.zero_()
            gx = model["cnet"].backward(x, [gb0, gc])
            gx_h = gx.numpy().copy()
            model["cnet"].join_backward()
            res.append((cls_h, gx_h, _host(g).copy()))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    (cls_p, gx_p, g_p), (cls_s, gx_s, g_s) = res
    assert same_bits(cls_p, cls_s) and np.array_equal(gx_p, gx_s) and gx_p.any()
    assert np.array_equal(g_p[:ow], g_s[:sow]) and np.array_equal(g_p[end:], g_s[send:]) and g_p[end:].any()
    assert not g_p[ow:end].any() and not g_s[sow:send].any()
    if layers:
        assert g_p[mp["native"].pnet_params:ow].any()


# ---- 2. one class: both layouts coincide ----------------------------------------------------------------------------------------
STEP_H, STEP_W = 225, 400     # (the frame of tests/test_gpu_roi_sampling.py: the sampler finds foreground rows on it)


def _one_step(F, box_head, rs):
    import torch
    model, w, g = tiny(F, 1, box_head)
    if rs is not None:
        model["cfg"]["roi_sampling"] = dict(rs)
    it = F.SyntheticBatchIterator(model, H=STEP_H, W=STEP_W, pool=2)
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    f = F.create_objective(model, w, g, it, stats)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        f(w)
        torch.cuda.synchronize()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    if rs is None:
        rec = f.debug["cnet_loss"]
        R, npos = rec["R"], rec["npos"]
    else:
        rec = f.debug["roi_sampling"]
        R, npos = rec["counts"][2] + rec["counts"][3], rec["counts"][2]
    rows = dict((k, rec[k].numpy()[:R].copy()) for k in ("crout", "crdelta", "cinput", "crtarget"))
    return dict(g=_host(g).copy(), w=_host(w).copy(), rows=rows, R=R, npos=npos, E=f.debug["E"], nat=model["native"],
                heads=model["pnet"].heads_param_range())


@pytest.mark.parametrize("rs", [None, dict(source="proposals", batch=64, fg_fraction=0.25, seed=3, post_nms_top_n=192)],
                         ids=["examples", "proposals"])
def test_one_class_step_agrees_with_the_shared_head(F, monkeypatch, rs):
    """class_count = 1: the per-class layout IS the shared one, so a per-class and a shared model run one deterministic step on the
    same flat weights (separate launches in both, so that only the box head's three launches differ).
    Everything in front of the head is bit-equal.  Foreground rows of crout: both sides are within the forward bound of the exact
    value, so they differ by at most twice the bound.  The box head's slice of the flat gradient: each side is within the
    weight-gradient bound of ITS exact sum, and the sums differ by the two sides' crdelta -- |d crdelta| <= 10 |d crout|
    (SmoothL1' is 1-Lipschitz, the factor 10 is objective.lua:172-173) -- all times the step's scale 1 / E, plus one rounding
    of that product.  The class head's and the anchor nets' slices do not depend on the box head: bit-equal.  The backbone and
    the rest receive the box head's input gradient (5 u per element, and d crdelta) through a linear map evaluated in fp32;
    no element-wise bound is derived for that map here: the slice is held to a norm-wise 1e-4 of its own size, a thousand times
    the perturbation's relative size."""
    monkeypatch.setenv("FRCNN_CNET_FUSE", "0")
    p, s = _one_step(F, PER, rs), _one_step(F, None, rs)
    assert p["nat"].desc.box_per_class == 1 and s["nat"].desc.box_per_class == 0
    assert same_bits(p["w"], s["w"]) and (p["R"], p["npos"], p["E"]) == (s["R"], s["npos"], s["E"]) and p["npos"] >= 2
    R, npos, E = p["R"], p["npos"], p["E"]
    ow, ob, end, nf, rows = head(p["nat"])
    assert rows == 4 and same_bits(p["rows"]["cinput"], s["rows"]["cinput"]) and same_bits(p["rows"]["crtarget"], s["rows"]["crtarget"])
    x = p["rows"]["cinput"]
    Wb, bb = p["w"][ow:ob].reshape(4, nf), p["w"][ob:end]
    sel = np.r_[np.ones(npos, np.int32), np.zeros(R - npos, np.int32)]
    out, mag = B.forward(x, Wb, bb, sel)
    fb = B.forward_bound(nf, mag)
    d_out = np.abs(p["rows"]["crout"].astype(np.float64) - s["rows"]["crout"])
    print("crout: per-class vs exact %.3g, shared vs exact %.3g, bound %.3g (largest, foreground rows)" % (
        np.abs(p["rows"]["crout"] - out)[:npos].max(), np.abs(s["rows"]["crout"] - out)[:npos].max(), fb[:npos].max()))
    assert np.all(np.abs(p["rows"]["crout"] - out)[:npos] <= fb[:npos]) and np.all(d_out[:npos] <= 2 * fb[:npos])
    assert not p["rows"]["crout"][npos:].any() and not s["rows"]["crout"][npos:].any()          # the losses zeroed them
    assert p["rows"]["crout"][:npos].any()
    # the box head's slice
    scale = np.float64(np.float32(1.0 / E))
    wg = B.weight_gradient(p["rows"]["crdelta"], x, sel, 1, np.zeros((4, nf)), np.zeros(4))
    assert int(wg["n"][0]) == npos
    for got, ref, m in ((p["g"][ow:ob].reshape(4, nf), wg["gW"], wg["magW"]), (p["g"][ob:end], wg["gb"], wg["magb"])):
        bound = B.weight_gradient_bound(npos, m) * scale + B.U * np.abs(ref * scale)       # (the per-class side against ITS sum)
        assert np.all(np.abs(got - ref * scale) <= bound)
    # crdelta = fl(10 fl(crout - target)) clamped to +-10: two roundings a side on top of 10 |d crout| -> 8 u |crdelta| covers them
    dg = np.abs(p["rows"]["crdelta"].astype(np.float64) - s["rows"]["crdelta"])
    assert np.all(dg[:npos] <= 10.0 * d_out[:npos] + 8 * B.U * np.abs(p["rows"]["crdelta"][:npos])) and not dg[npos:].any()
    # (the shared side's magnitudes are the per-class side's plus at most dg^T |x|: the factor on that term)
    bw = (2 * B.weight_gradient_bound(npos, wg["magW"]) + (dg.T @ np.abs(x.astype(np.float64))) * (1 + (npos + 2) * B.U)) \
        * scale * (1 + 2 * B.U) + 2 * B.U * np.abs(wg["gW"] * scale)
    assert np.all(np.abs(p["g"][ow:ob].astype(np.float64) - s["g"][ow:ob]).reshape(4, nf) <= bw) and p["g"][ow:ob].any()
    # independent of the box head: the class head, the anchor nets
    heads_lo, pn = p["heads"]
    assert pn == p["nat"].pnet_params
    assert same_bits(p["g"][end:], s["g"][end:]) and same_bits(p["g"][heads_lo:pn], s["g"][heads_lo:pn]) and p["g"][end:].any()
    # the backbone (see the docstring)
    a, b = p["g"][:heads_lo].astype(np.float64), s["g"][:heads_lo].astype(np.float64)
    rel = np.linalg.norm(a - b) / np.linalg.norm(b)
    print("backbone slice: relative difference %.3g" % rel)
    assert np.linalg.norm(b) > 0 and rel <= 1e-4


# ---- 3. key absent against {per_class = false} ----------------------------------------------------------------------------------
def test_absent_and_false_train_alike(F):
    import torch
    out = []
    for bh in (None, dict(per_class=False), {}):
        model, w, g = tiny(F, 3, bh, [dict(n=32, dropout=0.5)])
        it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
        f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
        state = dict(learningRate=1e-3)
        F._lib.call("frcnn_set_option", b"deterministic", 1)
        try:
            for k in range(2):
                F.rmsprop(f, w, state)
            torch.cuda.synchronize()
        finally:
            F._lib.call("frcnn_set_option", b"deterministic", 0)
        out.append((_host(w).copy(), model["native"].total_params))
    assert out[0][1] == out[1][1] == out[2][1]
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][0], out[2][0])


# ---- 4. the Detector, exact end to end ------------------------------------------------------------------------------------------
CLASSES = 4
SEEDS = list(range(5, 13))


def _bias(c, j):
    """class c's box: a different small shift and scale per class (exact in fp32)"""
    return [0.125 * c, -0.0625 * c, 0.03125 * (c - 2), 0.015625 * (3 - c)][j]


@pytest.fixture(scope="module")
def detector_setup(F):
    """a per-class vgg_small with four classes whose box-head weights are zero and whose biases differ per class: every product
    is exactly 0, so a row's box is its class's bias exactly.  The class head's gain is the first of GAINS that gives winners of
    at least two classes."""
    import torch
    cfg = dict(F.duplo_cfg, class_count=CLASSES, box_head=PER)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    nat = model["native"]
    ow, ob, end, nf, rows = head(nat)
    w0 = _host(weights).copy()
    w0[ow:ob] = 0.0
    w0[ob:end] = [_bias(c, j) for c in range(1, CLASSES + 1) for j in range(4)]
    frames = _frames(F, SEEDS, H, W)
    # An untrained class head predicts one class for every candidate.  Here its weight is a seeded normal draw, so that the
    # logits follow the candidates' features, and its bias is set from one pass over the frames so that every class's logit has
    # the mean of class 1's: the arg-max then varies from candidate to candidate.
    (cw, cn, _, _), (cb, cbn, _, _) = (tuple(int(v) for v in r) for r in nat.param_table[-2:])
    assert cn == (CLASSES + 1) * nf and cbn == CLASSES + 1
    w = _amplified_weights(nat, w0, CLASSES + 1, cls_gain=1.0)          # (the anchor nets' logits: p > 0.95 fires)
    w[cw:cw + cn] = np.random.RandomState(9).standard_normal(cn).astype(np.float32)
    w[cb:cb + cbn] = 0.0
    weights.copy_(torch.from_numpy(w))
    d = F.Detector(model)
    lps = []
    for f in frames:
        d.detect(f)
        if d.last_scan["n"]:
            lps.append(np.asarray(d.last_cnet["cls"], dtype=np.float64))
    lp = np.concatenate(lps)
    w[cb:cb + cbn] = -(lp - lp[:, :1]).mean(0).astype(np.float32)
    weights.copy_(torch.from_numpy(w))
    wins = [F.Detector(model).detect(f) for f in frames]
    present = sorted({x["class"] for win in wins for x in win})
    assert len(present) >= 2, "winners of %s only: the class head does not separate the candidates" % present
    shared = F.vgg_small(dict(F.duplo_cfg, class_count=CLASSES))
    sw, sg = F.combine_and_flatten_parameters(shared["pnet"], shared["cnet"], seed=42)
    print("detector: classes among the winners %s, candidates %d" % (present, len(lp)))
    return dict(model=model, weights=weights, w=w, shared=shared, sw=sw, frames=frames, present=present)


def _of_class(winners, c):
    return [r for r in _winner_rows(winners) if r[0] == c]


@pytest.mark.parametrize("mode", ["detect", "detect_batch", "box_voting"])
def test_detector_decodes_the_box_of_the_predicted_class(F, detector_setup, monkeypatch, mode):
    """for each class c among the winners: a shared-head model with zero weights and the bias of class c gives the same winners of
    class c -- rows, order, confidence, candidate, r and r2, bit for bit.  Both models run the class head as separate launches
    (FRCNN_CNET_FUSE=0): a per-class model always does, and the fused two-heads launch of the shared model sums the class
    logits in another order, which moves a confidence by a last bit."""
    import torch
    monkeypatch.setenv("FRCNN_CNET_FUSE", "0")
    s = detector_setup
    kw = dict(box_voting=dict(overlap=0.5)) if mode == "box_voting" else {}

    def run(model):
        d = F.Detector(model, **kw)
        return d.detect_batch(s["frames"]) if mode == "detect_batch" else [d.detect(f) for f in s["frames"]]
    got = run(s["model"])
    total = 0
    for c in s["present"]:
        s["sw"].copy_(torch.from_numpy(shared_weights(s["model"]["native"], s["w"], c)))
        want = run(s["shared"])
        for b, (g, r) in enumerate(zip(got, want)):
            assert _of_class(g, c) == _of_class(r, c), "class %d, frame %d" % (c, b)
            total += len(_of_class(g, c))
    assert total >= 2
    # the boxes differ between the classes: a shared head with ONE bias cannot give all of them
    rows = [r for win in got for r in _winner_rows(win)]
    assert len({r[0] for r in rows}) >= 2


def test_all_class_scoring_is_refused(F, detector_setup):
    s = detector_setup
    with pytest.raises(F.FrcnnError, match="box_head.per_class"):
        F.Detector(s["model"], scoring=dict(classes="all"))
    d = F.Detector(s["model"], scoring=dict(classes="top"))
    with pytest.raises(F.FrcnnError, match="scoring.classes"):
        d.set_scoring(dict(classes="all", min_confidence=0.05))
    assert d.scoring[0] == "top"


# ---- 5. optimisers and staged training on the longer vector ---------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_an_optimiser_step_moves_the_new_rows(F, opt):
    import torch
    model, w, g = tiny(F, 3, PER, [dict(n=32, dropout=0.5)])
    ow, ob, end, nf, rows = head(model["native"])
    assert rows == 12
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    w0 = _host(w).copy()
    if opt == "rmsprop":
        F.rmsprop(f, w, dict(learningRate=1e-3))
    else:
        F.adam(f, w, dict(learningRate=1e-3))
    torch.cuda.synchronize()
    w1, g1 = _host(w), _host(g)
    classes = sorted({int(c) for c in f.debug["cnet_loss"]["cctarget"].numpy()[:f.debug["cnet_loss"]["npos"]]})
    assert classes and all(1 <= c <= 3 for c in classes)
    moved = (w1[ow:ob] != w0[ow:ob]).reshape(rows, nf).any(1)
    want = np.repeat([c in classes for c in (1, 2, 3)], 4)
    assert np.array_equal(moved, want), (moved, classes)                # the rows of the classes in the batch, and only they
    # (a bias coordinate's gradient is a sum of a few clamped +-10 and may cancel to 0: some coordinate of each class present moves)
    moved_b = w1[ob:end] != w0[ob:end]
    assert not moved_b[~want].any() and np.array_equal(moved_b.reshape(3, 4).any(1), want[::4]) and np.isfinite(w1).all()
    assert (w1[end:] != w0[end:]).any() and (w1[:ow] != w0[:ow]).any()


def test_staged_training_without_the_classification_stage_leaves_the_rows(F):
    import torch
    model, w, g = tiny(F, 3, PER, [dict(n=32, dropout=0.5)])
    model["cfg"]["train"] = dict(proposal=True, classification=False, frozen_blocks=0)
    ow, ob, end, nf, rows = head(model["native"])
    pn = model["native"].pnet_params
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    w0 = _host(w).copy()
    F.rmsprop(f, w, dict(learningRate=1e-3))
    torch.cuda.synchronize()
    w1 = _host(w)
    assert same_bits(w1[pn:], w0[pn:]) and (w1[:pn] != w0[:pn]).any() and end <= model["native"].total_params
