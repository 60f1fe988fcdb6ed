"""Model-level parity on the GPU: pnet / cnet forward+backward, one full lossAndGradient
(objective.lua:45-218) and Detector:detect (Detector.lua:17-141) against the CPU oracle, at an
image size the oracle finishes in seconds (3x128x176, real vgg_small topology)."""
import numpy as np
import pytest

import decisions
from util import VGG_SMALL_CLS, VGG_SMALL_HEADS, VGG_SMALL_LAYERS, assert_close, oracle_model, oracle_tables

pytestmark = pytest.mark.gpu
H, W = 128, 176


@pytest.fixture(scope="module")
def setup(F, O):
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    om = oracle_model(O, cfg)
    w_host = weights.cpu().numpy().copy()
    assert O.param_count(om) == (model["native"].total_params, model["native"].pnet_params)
    assert model["native"].total_params == 26784106
    return dict(cfg=cfg, model=model, weights=weights, gradient=gradient, om=om, w=w_host)


def _masks(rng, model):
    return [None if l["dropout"] <= 0 else (rng.rand(l["filters"]) > l["dropout"]).astype(np.float32)
            for l in model["layers"]]


def check_pnet_forward_backward(F, O, s, img, masks, rng, what="pnet"):
    """pnet:forward / :backward with dense random deltas against the oracle, the device's discrete decisions (max-pool
    winners, PReLU branches) injected into the oracle (tests/decisions.py): outputs 1e-4, EVERY gradient tensor of the
    proposal net at SURVEY 8d's strict bars (1e-3 L2 per tensor + 1e-4 elementwise), nothing left out."""
    model = s["model"]
    pnet = model["pnet"]
    nat = model["native"]
    _, H, W = img.shape
    pnet.training()
    pnet.drop_masks = masks
    try:
        outs = pnet.forward(img)
        dec = decisions.capture(F, model, H, W)
        own = decisions.blank_like(dec)
        g_want = np.zeros_like(s["w"])
        with O.decisions(inject=dec, record=own):
            want, st = O.pnet_forward(s["om"], s["w"], img, True, masks)
            assert [o.shape for o in outs] == [w.shape for w in want]
            for i, (o, w) in enumerate(zip(outs, want)):
                assert_close(o.numpy(), w, 1e-4, "%s output %d" % (what, i + 1))
            deltas = [(rng.randn(*w.shape) / np.sqrt(w.size)).astype(np.float32) for w in want]
            O.pnet_backward(s["om"], s["w"], st, deltas, g_want)
        s["gradient"].zero_()
        dev_deltas = pnet.delta_outputs(zero=True)
        for d, h in zip(dev_deltas, deltas):
            d.copy_from_numpy(h)
        pnet.backward(img, dev_deltas)
        g = s["gradient"].cpu().numpy()
        _compare_gradient(nat, g, g_want, lo=0, hi=nat.pnet_params, slope_terms=decisions.slope_terms(nat, model, own["slope_abs"]))
        diff = decisions.count_differences(dec, own)
        print("%s %dx%d: decisions the oracle would have taken differently: %s" % (what, W, H, {k: "%d of %d" % v for k, v in diff.items()}))
        for kind, (nd, nt) in diff.items():
            assert nd <= max(4, 2e-5 * nt), (kind, nd, nt)
    finally:
        pnet.drop_masks = None
    return outs


def test_pnet_forward_backward(F, O, setup):
    s = setup
    rng = np.random.RandomState(0)
    img = F.synthetic_image(H, W, 0)
    check_pnet_forward_backward(F, O, s, img, _masks(rng, s["model"]), rng)
    pnet = s["model"]["pnet"]
    # evaluate(): SpatialDropout scales by (1-p)
    pnet.evaluate()
    outs = pnet.forward(img)
    want, _ = O.pnet_forward(s["om"], s["w"], img, False, None)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert_close(o.numpy(), w, 1e-4, "pnet eval output %d" % (i + 1))


def _compare_gradient(native, g, g_want, lo, hi, tol_l2=1e-3, elementwise=True, slope_terms=None):
    """1e-3 relative on the L2 norm per tensor + 1e-4 abs-or-relative elementwise, for every tensor of the
    parameter table whose offset lies in [lo, hi).  Every failing tensor is listed.
    slope_terms {offset: T}: a PReLU slope gradient is ONE number, the sum over a whole layer of terms x * gy of either
    sign; T = sum |x * gy| (from the oracle, tests/decisions.py).  The entries of gy are themselves only good to the
    elementwise bar, so the sum cannot be better than that bar times T: its tolerance is 1e-3 |b| + 1e-5 T (ten times
    tighter than 8d's 1e-4 elementwise bar applied to the terms)."""
    bad = []
    for off, cnt, kind, aux in native.param_table:
        if not (lo <= off < hi):
            continue
        a, b = g[off:off + cnt].astype(np.float64), g_want[off:off + cnt].astype(np.float64)
        nb = np.linalg.norm(b)
        err = np.linalg.norm(a - b)
        # absolute floor: tensors whose true gradient is ~0 (e.g. a Linear bias feeding BatchNorm) hold only
        # fp32 rounding noise of relative size 1e-6 of the neighbouring activations' gradients
        floor = 1e-5 * slope_terms[off] if slope_terms and off in slope_terms else 0.0
        if not err <= tol_l2 * nb + 1e-6 * np.sqrt(cnt) + floor:
            bad.append("tensor @%d kind %d (%d elements): |a-b|=%.3e |b|=%.3e" % (off, kind, cnt, err, nb))
        scale = max(1e-30, np.abs(b).max())
        if elementwise and not np.abs(a - b).max() <= 1e-4 * max(1.0, scale) + 1e-3 * scale + floor:   # (a slope is one element: same bar)
            bad.append("tensor @%d kind %d (%d elements) elementwise: max|a-b|=%.3e max|b|=%.3e" % (off, kind, cnt, np.abs(a - b).max(), scale))
    assert not bad, "\n".join(bad)


def test_cnet_forward_backward(F, O, setup):
    s = setup
    rng = np.random.RandomState(1)
    R, D = 37, 6 * 6 * 384
    x = rng.randn(R, D).astype(np.float32)
    cmasks = [(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)]
    cnet = s["model"]["cnet"]
    native = s["model"]["native"]
    bn0 = native.bn_running.cpu().numpy().copy()
    cnet.training()
    cnet.drop_masks = cmasks
    bbox, cls = cnet.forward(x)
    bn_o = bn0.copy()
    wb, wc, st = O.cnet_forward(s["om"], s["w"], x, True, cmasks, bn_o)
    assert_close(bbox.numpy(), wb, 1e-4, "cnet bbox")
    assert_close(cls.numpy(), wc, 1e-4, "cnet cls")
    assert_close(native.bn_running.cpu().numpy(), bn_o, 1e-5, "bn running stats")
    gb = rng.randn(R, 4).astype(np.float32); gc = (rng.randn(R, 17) / R).astype(np.float32)
    g_want = np.zeros_like(s["w"])
    gx_want = O.cnet_backward(s["om"], s["w"], st, gb, gc, g_want, D)
    s["gradient"].zero_()
    dgb, dgc = F.DeviceTensor.from_numpy(gb), F.DeviceTensor.from_numpy(gc)
    gx = cnet.backward(x, [dgb, dgc])
    assert_close(gx.numpy(), gx_want, 1e-4, "cnet gradInput")
    _compare_gradient(native, s["gradient"].cpu().numpy(), g_want, lo=native.pnet_params, hi=native.total_params)
    cnet.drop_masks = None
    cnet.evaluate()
    bbox, cls = cnet.forward(x)
    wb, wc, _ = O.cnet_forward(s["om"], s["w"], x, False, None, bn_o.copy())
    assert_close(bbox.numpy(), wb, 1e-4, "cnet eval bbox")
    assert_close(cls.numpy(), wc, 1e-4, "cnet eval cls")
    import torch
    native.bn_running.copy_(torch.from_numpy(bn0))


class _OneBatch(object):
    def __init__(self, batch, anchors):
        self.batch, self.anchors = batch, anchors

    def nextTraining(self, count=None):
        return self.batch


def check_loss_and_gradient(F, O, s, H, W, nimages=2, nrois=3, negatives=8, heads_lo=None, examples=None, pmasks=None):
    """objective.lua:45-218 on `nimages` images: losses within 1e-5 relative, gradient per SURVEY 8d.  `s`: dict with
    cfg, model, weights, gradient, om (oracle model), w (host copy of the weights).  `examples`: explicit images
    [(img, rois, positive, negative)], cleaned lists, in place of the sampled ones; `pmasks`: explicit SpatialDropout
    keep vectors of the proposal net in place of random ones."""
    model, cfg = s["model"], s["cfg"]
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    rng_m = np.random.RandomState(3)
    mt = F.MT19937(7)
    batch, oracle_in = [], []
    if examples is not None:
        oracle_in = list(examples)
        batch = [dict(img=img, positive=pos, negative=neg) for img, rois, pos, neg in oracle_in]
        nimages = len(batch)
    else:
        for k in range(nimages):
            rois = F.synthetic_rois(cfg, W, H, nrois, 7, k)
            pos, neg = F.assemble_examples(anchors, cfg, rois, W, H, mt, negatives=negatives)
            sizes = F.output_map_sizes(model, H, W)
            pos, neg = F.clean_examples(pos, sizes), F.clean_examples(neg, sizes)   # cleanAnchors, objective.lua:74-75
            img = F.synthetic_image(H, W, k)
            batch.append(dict(img=img, positive=pos, negative=neg))
            oracle_in.append((img, rois, pos, neg))
    assert sum(len(b["positive"]) for b in batch) > 0
    pm = _masks(rng_m, model) if pmasks is None else pmasks
    model["pnet"].drop_masks = pm
    nat = model["native"]
    n1, n2 = [l["n"] for l in model["class_layers"]]
    bn0 = nat.bn_running.cpu().numpy().copy()
    # explicit cnet masks per image (R differs): drawn once, handed to both sides
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    cm_per_image = []
    for (img, rois, pos, neg) in oracle_in:
        R = len(pos) + len(neg)
        cm_per_image.append([(rng_m.rand(R, n1) > 0.5).astype(np.float32), (rng_m.rand(R, n2) > 0.5).astype(np.float32)])

    cnet = model["cnet"]
    orig_forward = cnet.forward
    it = iter(cm_per_image)

    def fwd(x):   # per-image explicit masks: wrap cnet.forward to install them in order
        cnet.drop_masks = next(it)
        return orig_forward(x)
    cnet.forward = fwd
    try:
        f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
        # the device's discrete decisions (pool winners, PReLU branches, ROI cell winners) of every image, copied out
        # right before that image's backward pass
        with decisions.CaptureBeforeBackward(F, model, f) as cap:
            loss, grad = f(s["weights"])
    finally:
        cnet.forward = orig_forward
        cnet.drop_masks = None
        model["pnet"].drop_masks = None
    assert len(cap.captured) == nimages
    # ---- the oracle, taking those decisions as given (and recording the ones it would have taken itself) -------------
    g_want = np.zeros_like(s["w"]); acc = np.zeros(8); bn_o = bn0.copy()
    differing = {}
    slope_abs = np.zeros(48)
    for k, (img, rois, pos, neg) in enumerate(oracle_in):
        own = decisions.blank_like(cap.captured[k])
        own["slope_abs"] = slope_abs      # (accumulates over the images like the gradient itself)
        with O.decisions(inject=cap.captured[k], record=own):
            O.train_image(s["om"], s["w"], g_want, img, *oracle_tables(pos, neg, rois), pm, cm_per_image[k], bn_o, acc)
        for kind, (nd, nt) in decisions.count_differences(cap.captured[k], own).items():
            a, b = differing.get(kind, (0, 0))
            differing[kind] = (a + nd, b + nt)
    g_want /= acc[2]
    want = dict(pcls=acc[0] / acc[2], preg=acc[1] / acc[3], dcls=acc[6] / acc[7], dreg=acc[4] / acc[5])
    for k in ("pcls", "preg", "dcls", "dreg"):
        assert abs(stats[k][-1] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, stats[k][-1], want[k])
    assert abs(loss - (want["pcls"] + want["preg"])) <= 1e-5 * max(1.0, abs(loss))
    # SURVEY 8d's bars on EVERY tensor of the flat gradient -- 1e-3 relative on the L2 norm per tensor, 1e-4 elementwise --
    # no tensor left out, no row set aside: with the routes fixed, what is compared is arithmetic.
    _compare_gradient(nat, grad.cpu().numpy(), g_want, 0, nat.total_params, tol_l2=1e-3, elementwise=True,
                      slope_terms=decisions.slope_terms(nat, model, slope_abs, acc[2]))
    lo = model["pnet"].heads_param_range()[0]
    if heads_lo is not None:
        assert lo == heads_lo
    # How many decisions the fp64-accumulating restatement takes differently from the fp32 device (values within rounding
    # of each other / of zero): a handful per million, reported and bounded.
    print("decisions taken differently by the oracle: %s" % {k: "%d of %d" % v for k, v in differing.items()})
    for kind, (nd, nt) in differing.items():
        assert nd <= max(4, 2e-5 * nt), (kind, nd, nt)
    assert_close(nat.bn_running.cpu().numpy(), bn_o, 1e-5, "bn running")
    import torch
    nat.bn_running.copy_(torch.from_numpy(bn0))
    return dict(loss=loss, examples=int(acc[2]))


def test_loss_and_gradient(F, O, setup):
    """objective.lua:45-218 on two images: losses within 1e-5 relative, gradient per SURVEY 8d."""
    check_loss_and_gradient(F, O, setup, H, W, heads_lo=3321095)


def _amplified_weights(nat, w, ncls, cls_gain=30.0):
    """Head logits amplified so that the p > 0.95 test fires, class head sharpened so that p > 0.2 does."""
    w = w.copy()
    for off, cnt, kind, aux in nat.param_table:
        if kind == 0 and aux == 18:  # the 1x1 head convs (kW*kH*nOutputPlane = 18): amplify the 2 class logits
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= 60.0
        if kind == 3 and cnt == 512 * ncls:  # class head of cnet: make the arg-max confident (p > 0.2)
            w[off:off + cnt] *= cls_gain
    return w


def _iou_border_pairs(boxes, thr, eps=1e-5):
    """number of box pairs whose nms.lua IoU (the +1 convention of nms.lua:35,88-94) lies within eps of thr"""
    b = boxes.astype(np.float64)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    n = 0
    for lo in range(0, len(b), 512):
        c = b[lo:lo + 512]
        w = np.maximum(0, np.minimum(c[:, None, 2], b[None, :, 2]) - np.maximum(c[:, None, 0], b[None, :, 0]) + 1)
        h = np.maximum(0, np.minimum(c[:, None, 3], b[None, :, 3]) - np.maximum(c[:, None, 1], b[None, :, 1]) + 1)
        inter = w * h
        iou = inter / (area[lo:lo + 512, None] + area[None, :] - inter)
        n += int((np.abs(iou - thr) < eps).sum())
    return n


def check_detect(F, O, model, om, w, img_seeds, H, W):
    """Detector:detect against the oracle on EVERY frame of `img_seeds`, every stage.  A stage's lists may differ between
    the fp32 device and the fp64-accumulating restatement only where a BORDER CASE is shown to exist -- an anchor whose
    probability lies within 1e-4 of the 0.95 threshold (Detector.lua:54), a pair of boxes whose IoU lies within 1e-5 of the
    NMS threshold (:81) -- and the test asserts that: without such a case the lists must be identical, and once they are,
    everything downstream (decoded rects, cnet outputs, winners with their boxes) is compared, unconditionally.  NMS ids on
    identical boxes are always bit-exact.  At least one frame must go all the way."""
    nat = model["native"]
    d = F.Detector(model)
    bn = nat.bn_running.cpu().numpy()
    deep = []
    for seed in img_seeds:
        img = F.synthetic_image(H, W, seed)
        winners = d.detect(img)
        ref = O.detect(om, w, bn, img)
        m = d.last_scan
        gp, gidx, grect = m["p"].numpy(), m["idx"].numpy(), m["rect"].numpy()

        def key(a):
            return set(map(tuple, a.tolist()))
        # matches: identical anchor indices except those within 1e-4 of the 0.95 threshold
        border_ref = np.abs(np.exp(ref["match_p"].astype(np.float64)) - 0.95) < 1e-4
        border_got = np.abs(np.exp(gp.astype(np.float64)) - 0.95) < 1e-4
        assert key(gidx[~border_got]) - key(ref["match_idx"]) == set()
        assert key(ref["match_idx"][~border_ref]) - key(gidx) == set()
        assert len(gidx) > 10, "test image produced too few matches to be meaningful"
        same_matches = len(gidx) == len(ref["match_idx"]) and np.array_equal(gidx, ref["match_idx"])
        if not (border_ref.any() or border_got.any()):
            assert same_matches, "frame %d: match lists differ although no anchor is near the threshold" % seed
        # NMS ids: bit-exact when the oracle NMS is fed the boxes the GPU produced
        boxes = m["box"].numpy()
        assert d.last_pick.tolist() == O.nms(boxes, 0.25).tolist()
        if not same_matches:
            print("frame %d: %d / %d border anchors, match lists differ by them only" % (seed, border_got.sum(), border_ref.sum()))
            continue
        assert_close(gp, ref["match_p"], 1e-4, "match log-prob")
        assert_close(grect, ref["match_rect"], 1e-3, "decoded rects")
        same_picks = d.last_pick.tolist() == ref["cand_ids"].tolist()
        if not same_picks:
            nb = _iou_border_pairs(boxes, 0.25)
            assert nb > 0, "frame %d: NMS candidates differ although no box pair is near the overlap threshold" % seed
            print("frame %d: %d box pairs within 1e-5 of the NMS threshold, candidate lists differ" % (seed, nb))
            continue
        assert len(ref["cand_ids"]) > 0
        assert_close(d.last_cnet["bbox"], ref["cand_bbox"], 1e-3, "cnet bbox (eval)")
        assert_close(d.last_cnet["cls"], ref["cand_cls"], 1e-3, "cnet log-probs (eval)")
        # winners: {class, confidence, r2} per class in NMS pick order (classes ascending on both sides).  Border cases of
        # this stage: a candidate whose top two class log-probabilities agree to 1e-4, or whose confidence lies within 1e-4
        # of 0.2 (Detector.lua:110-115)
        cls_sorted = np.sort(ref["cand_cls"].astype(np.float64), axis=1)
        cls_border = int(((cls_sorted[:, -1] - cls_sorted[:, -2]) < 1e-4).sum() + (np.abs(np.exp(cls_sorted[:, -1]) - 0.2) < 1e-4).sum())
        got_cls = [x["class"] for x in winners]; want_cls = [int(r[0]) for r in ref["winners"]]
        if got_cls != want_cls:
            wb = np.array([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], dtype=np.float32)
            assert cls_border > 0 or _iou_border_pairs(wb, 0.1) > 0, "frame %d: winners differ without a border case" % seed
            print("frame %d: winners differ by border cases" % seed)
            continue
        if len(winners):
            assert_close([x["confidence"] for x in winners], ref["winners"][:, 1], 1e-3, "winner confidence")
            assert_close([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], ref["winners"][:, 2:6],
                         1e-3, "winner rects (Detector.lua:107)")
        deep.append(dict(seed=seed, matches=len(gp), candidates=len(ref["cand_ids"]), winners=len(winners), ref=ref, got=winners))
    assert deep, "no frame of %r went through every stage" % (list(img_seeds),)
    print("detect: %d of %d frames compared through every stage" % (len(deep), len(list(img_seeds))))
    best = max(deep, key=lambda r: r["winners"])
    best["frames_compared"] = len(deep)
    return best


def test_detect(F, O, setup):
    """Detector:detect vs the oracle: matches, decoded rects, NMS picks, cnet outputs and the per-class winners."""
    s = setup
    import torch
    model = s["model"]
    nat = model["native"]
    w = _amplified_weights(nat, s["w"], 17, cls_gain=200.0)
    s["weights"].copy_(torch.from_numpy(w))
    try:
        r = check_detect(F, O, model, s["om"], w, range(5, 10), H, W)
        assert r["winners"] > 0, "no winner: the back half of detect was not exercised"
        print("detect: frame %(seed)d, %(matches)d matches, %(candidates)d candidates, %(winners)d winners" % r)
    finally:
        s["weights"].copy_(torch.from_numpy(s["w"]))


def test_cnet_fused_layers_equal_separate_launches(F, setup, monkeypatch):
    """Round 4: fold + BatchNormalization + PReLU + Dropout as one launch per layer (and their backward, and the class head's
    fold + LogSoftMax) against one launch per operation (FRCNN_CNET_FUSE=0): same arithmetic, the fp64 column sums of the
    batch normalisation meet in a different tree -- outputs, input gradient and the classification net's gradient within 1e-6."""
    s = setup
    model = s["model"]
    cnet, nat = model["cnet"], model["native"]
    rng = np.random.RandomState(21)
    import torch
    bn0 = nat.bn_running.cpu().numpy().copy()
    for R in (37, 300):   # below / above the row count from which the large Linear takes the split-bf16 form
        x = F.DeviceTensor.from_numpy(rng.randn(R, 13824).astype(np.float32))
        masks = [(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)]
        gb = F.DeviceTensor.from_numpy(rng.randn(R, 4).astype(np.float32))
        gc = F.DeviceTensor.from_numpy((rng.randn(R, 17) / R).astype(np.float32))
        res = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("FRCNN_CNET_FUSE", mode)
            nat.bn_running.copy_(torch.from_numpy(bn0))
            cnet.training()
            cnet.drop_masks = masks
            try:
                bbox, cls = cnet.forward(x)
                s["gradient"].zero_()
                gx = cnet.backward(x, [gb, gc])
                res[mode] = (bbox.numpy().copy(), cls.numpy().copy(), gx.numpy().copy(), s["gradient"].cpu().numpy().copy(),
                             nat.bn_running.cpu().numpy().copy())
            finally:
                cnet.drop_masks = None
        monkeypatch.delenv("FRCNN_CNET_FUSE", raising=False)
        a, b = res["1"], res["0"]
        for i, what in enumerate(("bbox", "log-probabilities", "input gradient")):
            assert_close(a[i], b[i], 1e-6, "%s (R = %d)" % (what, R))
        assert_close(a[4], b[4], 1e-6, "bn running statistics")
        ga, gb_ = a[3][nat.pnet_params:], b[3][nat.pnet_params:]
        assert np.abs(ga).max() > 0
        assert np.linalg.norm(ga - gb_) <= 1e-6 * np.linalg.norm(gb_), (R, np.linalg.norm(ga - gb_) / np.linalg.norm(gb_))
    nat.bn_running.copy_(torch.from_numpy(bn0))


def test_detect_first_nms_bound(F, setup):
    """Detector.NMS_FIRST_CAP: the first NMS launch is sized for a bound on the matches; a frame with more matches than
    the bound repeats the pass sized by the count read back.  Same candidates, same winners either way."""
    import torch
    s = setup
    model = s["model"]
    w = _amplified_weights(model["native"], s["w"], 17, cls_gain=200.0)
    s["weights"].copy_(torch.from_numpy(w))
    try:
        img = F.synthetic_image(H, W, 5)
        res = []
        for bound in (16384, 8):
            d = F.Detector(model)
            d.NMS_FIRST_CAP = bound
            win = d.detect(img)
            assert d.last_scan["n"] > 8
            res.append((d.last_pick.tolist(), [(x["class"], x["confidence"], x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY) for x in win]))
        assert len(res[0][0]) > 0
        assert res[0] == res[1]
    finally:
        s["weights"].copy_(torch.from_numpy(s["w"]))


def test_static_weights_reuses_packs_until_told(F, setup):
    """Option static_weights: evaluate-mode passes re-use the packed weight copies -- same detections as with the copies remade
    per frame; after the host writes the weights and says so (the option set again) the new weights are in effect."""
    import torch
    s = setup
    model = s["model"]
    w = _amplified_weights(model["native"], s["w"], 17, cls_gain=200.0)

    def run(det, img):
        win = det.detect(img)
        return det.last_pick.tolist(), det.last_scan["p"].numpy().copy(), [(x["class"], x["confidence"]) for x in win]
    try:
        s["weights"].copy_(torch.from_numpy(w))
        imgs = [F.synthetic_image(H, W, k) for k in (5, 6)]
        plain = F.Detector(model)
        want = [run(plain, im) for im in imgs]
        d = F.Detector(model, static_weights=True)
        for _ in range(2):   # (second round: the packs of the first are re-used)
            got = [run(d, im) for im in imgs]
            for a, b in zip(got, want):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
        # new weights: without a word the stale packs would still be used (that is the contract) -- the host says so
        w2 = w.copy(); w2[:model["native"].pnet_params] *= np.float32(0.5)
        s["weights"].copy_(torch.from_numpy(w2))
        F._lib.call("frcnn_set_option", b"static_weights", 1)
        after = run(d, imgs[0])
        F._lib.call("frcnn_set_option", b"static_weights", 0)
        fresh = run(F.Detector(model), imgs[0])
        assert after[0] == fresh[0] and np.array_equal(after[1], fresh[1])
        assert not np.array_equal(after[1], want[0][1]) or len(after[1]) != len(want[0][1])
    finally:
        F._lib.call("frcnn_set_option", b"static_weights", 0)
        s["weights"].copy_(torch.from_numpy(s["w"]))


def test_sparse_head_backward_equals_dense(F, setup):
    """frcnn_pnet_set_sparse_deltas: the anchor-head backward restricted to the non-zero delta positions must
    give the gradient of the dense backward (same arithmetic on fewer pixels; fp32 summation order differs)."""
    import ctypes as C
    s = setup
    rng = np.random.RandomState(5)
    model, nat = s["model"], s["model"]["native"]
    pnet = model["pnet"]
    pnet.training()
    pnet.drop_masks = _masks(rng, model)
    img = F.synthetic_image(H, W, 2)
    outs = pnet.forward(img)
    deltas_h, pos = [], []
    for l in range(4):
        c, h, w = outs[l].shape
        d = np.zeros((c, h * w), np.float32)
        n = [23, 5, 0, 1][l]                         # incl. a head without any example and a single position
        p = np.sort(rng.choice(h * w, n, replace=False)).astype(np.int32)
        d[:, p] = rng.randn(c, n).astype(np.float32)
        deltas_h.append(d.reshape(c, h, w)); pos.append(p)
    deltas_h.append((rng.randn(*outs[4].shape) * 0.01).astype(np.float32))

    def run(sparse):
        s["gradient"].zero_()
        dd = pnet.delta_outputs(zero=True)
        for d, hst in zip(dd, deltas_h):
            d.copy_from_numpy(hst)
        keep = []
        if sparse:
            for l in range(4):
                dp = F.DeviceTensor.from_numpy(pos[l]) if len(pos[l]) else None
                keep.append(dp)
                F._lib.call("frcnn_pnet_set_sparse_deltas", nat.h, l + 1, F.ptr(dp), len(pos[l]))
        pnet.backward(img, dd)
        return s["gradient"].cpu().numpy().copy()
    g_dense, g_sparse = run(False), run(True)
    pnet.drop_masks = None
    _compare_gradient(nat, g_sparse, g_dense, 0, nat.pnet_params, tol_l2=1e-5, elementwise=False)


def test_fused_activation_backward_equals_unfused(F, setup, monkeypatch):
    """Round 4: the PReLU / SpatialDropout / max-pooling backward folded into the neighbouring convolution launches (conv_x3's
    X3PostAct; the first layer's weight gradient straight from the pooled gradient, conv_wgrad_first_pooled) against the same
    pass with every activation backward as a launch of its own (FRCNN_FUSE_ACT=0): the whole proposal-net gradient, 1e-5 L2
    (the sums differ in order only), at an even and at an odd image size (ceil-mode pooling windows cut by the border)."""
    s = setup
    model = s["model"]
    pnet, nat = model["pnet"], model["native"]
    rng = np.random.RandomState(9)
    # (both passes dense: leaving out the dropped channels -- option drop_compact, tests/test_gpu_dropcompact.py -- needs the
    # fused form, and its other rounding would flip a pooling winner now and then, which is not what this test compares)
    for (h, w) in ((H, W), (117, 155)):
        img = F.synthetic_image(h, w, 2)
        pnet.training()
        pnet.drop_masks = _masks(rng, model)
        F._lib.call("frcnn_set_option", b"drop_compact", 0)
        try:
            outs = pnet.forward(img)
            deltas = [(rng.randn(*o.shape) / np.sqrt(o.numel())).astype(np.float32) for o in outs]
            res = {}
            for mode in ("1", "0"):
                monkeypatch.setenv("FRCNN_FUSE_ACT", mode)
                pnet.forward(img)
                s["gradient"].zero_()
                dd = pnet.delta_outputs(zero=True)
                for d, hst in zip(dd, deltas):
                    d.copy_from_numpy(hst)
                pnet.backward(img, dd)
                res[mode] = s["gradient"].cpu().numpy().copy()
        finally:
            pnet.drop_masks = None
            monkeypatch.delenv("FRCNN_FUSE_ACT", raising=False)
            F._lib.call("frcnn_set_option", b"drop_compact", 1)
        assert np.abs(res["1"][:nat.pnet_params]).max() > 0
        _compare_gradient(nat, res["1"], res["0"], 0, nat.pnet_params, tol_l2=1e-5, elementwise=False)


def test_side_stream_equals_serial(F, setup):
    """frcnn_set_option("side_stream"): issuing the anchor nets / weight gradients on the library's second
    stream (and starting the anchor nets' backward early, frcnn_pnet_backward_heads_begin) must not change the
    result: same losses, same gradient up to the summation order of delta_outputs[5] + anchor-net terms."""
    import torch
    s = setup
    model, cfg = s["model"], s["cfg"]
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    rois = F.synthetic_rois(cfg, W, H, 3, 7, 1)
    pos, neg = F.assemble_examples(anchors, cfg, rois, W, H, F.MT19937(11), negatives=8)
    sizes = F.output_map_sizes(model, H, W)
    pos, neg = F.clean_examples(pos, sizes), F.clean_examples(neg, sizes)
    batch = [dict(img=F.synthetic_image(H, W, 1), positive=pos, negative=neg)]
    R = len(pos) + len(neg)
    assert R > 0
    rng = np.random.RandomState(5)
    nat = model["native"]
    bn0 = nat.bn_running.cpu().numpy().copy()
    model["pnet"].drop_masks = _masks(rng, model)
    model["cnet"].drop_masks = [(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)]
    res = {}
    try:
        for mode in (1, 0):
            F._lib.call("frcnn_set_option", b"side_stream", mode)
            stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
            f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
            loss, grad = f(s["weights"])
            res[mode] = (loss, [stats[k][-1] for k in ("pcls", "preg", "dcls", "dreg")], grad.cpu().numpy().copy())
            nat.bn_running.copy_(torch.from_numpy(bn0))
    finally:
        F._lib.call("frcnn_set_option", b"side_stream", 1)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
    # (the cnet GEMMs accumulate their K splits with fp32 atomics: sums may differ in the last ulp between runs)
    assert abs(res[1][0] - res[0][0]) <= 1e-6 * abs(res[0][0])
    assert np.allclose(res[1][1], res[0][1], rtol=1e-6, atol=0)
    a, b = res[1][2], res[0][2]
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b), np.linalg.norm(a - b) / np.linalg.norm(b)


def test_bucketed_exchange_path_on_one_gpu(F, setup, monkeypatch):
    """The data-parallel code path of lossAndGradient (early all-reduce buckets for the cnet slice and, after
    frcnn_pnet_backward_heads_join, the anchor nets' slice; the rest + the 8 accumulators at the end) with an
    identity 'all-reduce': the result must equal the single-process result, and every element of the gradient
    must have been exchanged exactly once."""
    import torch
    from importlib import import_module
    obj = import_module(F.create_objective.__module__)
    s = setup
    model, cfg = s["model"], s["cfg"]
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    rois = F.synthetic_rois(cfg, W, H, 3, 7, 2)
    pos, neg = F.assemble_examples(anchors, cfg, rois, W, H, F.MT19937(13), negatives=8)
    sizes = F.output_map_sizes(model, H, W)
    pos, neg = F.clean_examples(pos, sizes), F.clean_examples(neg, sizes)
    batch = [dict(img=F.synthetic_image(H, W, 2), positive=pos, negative=neg)]
    R = len(pos) + len(neg)
    rng = np.random.RandomState(9)
    nat = model["native"]
    bn0 = nat.bn_running.cpu().numpy().copy()
    model["pnet"].drop_masks = _masks(rng, model)
    model["cnet"].drop_masks = [(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)]

    class _Work(object):
        def wait(self):
            return True

    class _FakeDist(object):
        def __init__(self):
            self.ranges = []

        def all_reduce(self, t, async_op=False):
            if t.dtype == torch.float32:
                base = s["gradient"].data_ptr()
                lo = (t.data_ptr() - base) // 4
                self.ranges.append((lo, lo + t.numel()))
            return _Work()

    try:
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
        loss0, grad = f(s["weights"])
        g0 = grad.cpu().numpy().copy()
        nat.bn_running.copy_(torch.from_numpy(bn0))
        fake = _FakeDist()
        monkeypatch.setattr(obj, "_dist", lambda: fake)
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
        loss1, grad = f(s["weights"])
        g1 = grad.cpu().numpy().copy()
        first_ranges = list(fake.ranges)
        # one optimiser step through utilities.rmsprop (begin_fold protocol: gradient:div folded into the update) in
        # both modes: identical weights afterwards
        w_start = s["weights"].clone()
        upd = {}
        for mode, dist_fn in (("dp", lambda: fake), ("single", lambda: None)):
            monkeypatch.setattr(obj, "_dist", dist_fn)
            stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
            f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
            F.rmsprop(f, s["weights"], dict(learningRate=1e-4, alpha=0.9))
            upd[mode] = s["weights"].cpu().numpy().copy()
            s["weights"].copy_(w_start)
            nat.bn_running.copy_(torch.from_numpy(bn0))
        assert np.abs(upd["dp"] - w_start.cpu().numpy()).max() > 0
        # (the first RMSprop step is lr * g / (sqrt(0.1 g^2) + eps) ~ lr * sign(g) / sqrt(0.1): elements whose gradient is
        # ~0 may flip with the last-ulp differences between the two runs, so compare against the size of the update)
        w0 = w_start.cpu().numpy()
        assert np.linalg.norm(upd["dp"] - upd["single"]) <= 1e-3 * np.linalg.norm(upd["single"] - w0)
    finally:
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
        nat.bn_running.copy_(torch.from_numpy(bn0))
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0)
    assert np.linalg.norm(g1 - g0) <= 1e-6 * np.linalg.norm(g0)
    # coverage: the buckets tile [0, n) exactly once; the early ones are the cnet slice and the anchor nets' slice
    r = sorted(first_ranges)
    assert r[0][0] == 0 and r[-1][1] == nat.total_params
    assert all(a[1] == b[0] for a, b in zip(r[:-1], r[1:])), r
    lo, hi = model["pnet"].heads_param_range()
    assert (nat.pnet_params, nat.total_params) in first_ranges and (lo, hi) in first_ranges and lo == 3321095
    # ... and the two deep backbone blocks, started behind frcnn_pnet_wait_block_gradients beside the rest of the pass
    b3, b2 = model["pnet"].block_param_range(3), model["pnet"].block_param_range(2)
    assert b3 in first_ranges and b2 in first_ranges and b3[1] == lo and b2[1] == b3[0]
    assert b3[1] - b3[0] == 256 * 384 * 9 + 384 * 384 * 9 + 2 * (384 + 1)


def test_deterministic_mode_is_bit_reproducible(F, setup):
    """frcnn_set_option("deterministic", 1): no floating-point partial results meet in fp32 atomics any more (ordered folds,
    gathers, 64-bit fixed point), so two runs of the same training step are BIT-identical -- and agree with the default mode
    to rounding."""
    import ctypes as C
    import torch
    s = setup
    model, cfg = s["model"], s["cfg"]
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    rois = F.synthetic_rois(cfg, W, H, 3, 7, 4)
    pos, neg = F.assemble_examples(anchors, cfg, rois, W, H, F.MT19937(17), negatives=24)
    sizes = F.output_map_sizes(model, H, W)
    pos, neg = F.clean_examples(pos, sizes), F.clean_examples(neg, sizes)
    neg = neg + neg[:5]          # the same anchor sampled twice (two deltas land on one address)
    batch = [dict(img=F.synthetic_image(H, W, 4), positive=pos, negative=neg)]
    R = len(pos) + len(neg)
    rng = np.random.RandomState(2)
    nat = model["native"]
    bn0 = nat.bn_running.cpu().numpy().copy()
    w0 = s["weights"].clone()
    model["pnet"].drop_masks = _masks(rng, model)
    model["cnet"].drop_masks = [(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)]
    runs = {}
    F._lib.call("frcnn_set_option", b"drop_compact", 0)   # (the deterministic pass is dense; "default" is compared with it to rounding)
    try:
        for tag, det in (("det_a", 1), ("det_b", 1), ("default", 0)):
            F._lib.call("frcnn_set_option", b"deterministic", det)
            v = C.c_int(-1)
            F._lib.call("frcnn_get_option", b"deterministic", C.byref(v))
            assert v.value == det
            stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
            f = F.create_objective(model, s["weights"], s["gradient"], _OneBatch(batch, anchors), stats)
            F.rmsprop(f, s["weights"], dict(learningRate=1e-4, alpha=0.9))
            torch.cuda.synchronize()
            runs[tag] = (s["gradient"].cpu().numpy().copy(), s["weights"].cpu().numpy().copy(), [stats[k][-1] for k in ("pcls", "preg", "dcls", "dreg")])
            s["weights"].copy_(w0)
            nat.bn_running.copy_(torch.from_numpy(bn0))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        F._lib.call("frcnn_set_option", b"drop_compact", 1)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
        s["weights"].copy_(w0)
        nat.bn_running.copy_(torch.from_numpy(bn0))
    assert np.array_equal(runs["det_a"][0], runs["det_b"][0]), "gradient differs between two deterministic runs"
    assert np.array_equal(runs["det_a"][1], runs["det_b"][1]), "updated weights differ between two deterministic runs"
    assert runs["det_a"][2] == runs["det_b"][2]
    g, gd = runs["default"][0].astype(np.float64), runs["det_a"][0].astype(np.float64)
    assert np.isfinite(gd).all() and np.abs(gd).max() > 0
    assert np.linalg.norm(g - gd) <= 1e-6 * np.linalg.norm(g)
    assert np.allclose(runs["default"][2], runs["det_a"][2], rtol=1e-6, atol=0)
