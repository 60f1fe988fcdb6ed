"""Training the classification net on sampled RPN proposals (cfg["roi_sampling"]) at 225x400 on vgg_small, deterministic mode,
explicit dropout masks (the set-up of tests/test_gpu_stages.py): with the key absent, empty or source = "examples" the step is
the parent's bit for bit and launch for launch; under "proposals" the sampler's recorded outputs equal the numpy restatement
applied to the recorded candidates and the entry's ground truth, the pooled rows are those of the recorded rects, the anchor
nets' part of the step is untouched, and the detector's statistics are those of the sampled rows."""
import ctypes as C

import numpy as np
import pytest

import proposal_targets_ref as R
from anchor_ops_ref import cnet_losses_ref
from test_gpu_optim import _host, same_bits
from test_gpu_stages import ROWS, _frozen, _groups, _setup

pytestmark = pytest.mark.gpu

H, W = 225, 400
ABSENT = "absent"
PROPOSALS = dict(source="proposals", batch=64, fg_fraction=0.25, seed=3)


def _counted(F, fn):
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        res = fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return res, list(la)


def _step(F, rs=ABSENT, train=None, roi_pooling=None, edit=None, steps=1, run=None, det=1):
    """`steps` lossAndGradient calls under cfg.roi_sampling = rs -> dict(g, stats, bn, model, f, it); the dropout masks are the
    same for every setting (the classification net's have rows for the largest batch of rows any of them can make)"""
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    cfg = model["cfg"]
    if rs is not ABSENT:
        cfg["roi_sampling"] = rs
    if train is not None:
        cfg["train"] = dict(train)
    if roi_pooling is not None:
        cfg["roi_pooling"] = dict(cfg["roi_pooling"], **roi_pooling)
        f = F.create_objective(model, w, g, it, stats)
    if edit is not None:
        edit(it)
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", det)
    try:
        for k in range(steps):
            model["pnet"].drop_masks = [None] + [(rng.rand(c) > 0.4).astype(np.float32) for c in (128, 256, 384)]
            model["cnet"].drop_masks = [(rng.rand(256, 1024) > 0.5).astype(np.float32), (rng.rand(256, 512) > 0.5).astype(np.float32)]
            (run or (lambda f, w: f(w)))(f, w)
        torch.cuda.synchronize()
        bn = model["native"].bn_running.cpu().numpy().copy()
        return dict(g=_host(g).copy(), stats=stats, bn=bn, model=model, f=f, it=it, w=w)
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None


@pytest.fixture(scope="module")
def plain(F):
    return _counted(F, lambda: _step(F))


@pytest.fixture(scope="module")
def sampled(F):
    return _counted(F, lambda: _step(F, PROPOSALS))


@pytest.mark.parametrize("rs", [{}, dict(source="examples"), dict(source="examples", batch=16, threshold=0.9)], ids=["empty", "examples", "examples_other_values"])
def test_examples_source_is_the_parent_step(F, plain, rs):
    (a, la), (b, lb) = plain, _counted(F, lambda: _step(F, rs))
    assert same_bits(a["g"], b["g"]) and same_bits(a["bn"], b["bn"])
    assert a["stats"] == b["stats"] and "rois" not in b["stats"]
    assert la == lb, "launches per class differ: %r vs %r" % (la, lb)
    assert "roi_sampling" not in b["f"].debug


def _case_of(rec, **kw):
    """the recorded candidates and ground truth as a case of proposal_targets_ref"""
    rs = rec["settings"]
    return dict(rect=rec["rect"].numpy(), pick=rec["pick"].numpy(), r_dev=int(rec["R"].numpy()[0]), r_cap=rec["r_cap"],
                gt_rect=rec["gt_rect"], gt_class=rec["gt_class"], include_gt=rs["include_gt"], fg_iou=rs["fg_iou"], bg_lo=rs["bg_iou"][0],
                bg_hi=rs["bg_iou"][1], fg_quota=rs["fg_quota"], batch=rs["batch"], bgclass=rec["bgclass"], seed=rec["seed"], name="recorded", **kw)


def _check_record(rec, entry):
    """the sampler's outputs == the restatement on its recorded inputs; the ground truth is the entry's"""
    assert rec["gt_rect"].tolist() == [[r.rect.minX, r.rect.minY, r.rect.maxX, r.rect.maxY] for r in entry["rois"]]
    assert rec["gt_class"].tolist() == [r.class_index for r in entry["rois"]]
    want = R.targets_ref(_case_of(rec))
    assert rec["counts"] == want["counts"]
    S = want["counts"][2] + want["counts"][3]
    for name in ("src", "gt_idx", "cctarget", "roi", "iou"):
        assert rec[name].numpy()[:S].tobytes() == want[name].tobytes(), name
    got = rec["crtarget"].numpy()[:S]
    assert got[:, :2].tobytes() == want["crtarget"][:, :2].tobytes()
    d = np.abs(got[:, 2:].view(np.int32).astype(np.int64) - want["crtarget"][:, 2:].view(np.int32).astype(np.int64))
    assert d.max(initial=0) <= 1
    return want, S


def test_sampler_outputs_equal_the_restatement(F, sampled, plain):
    (b, lb), (a, la) = sampled, plain
    rec = b["f"].debug["roi_sampling"]
    want, S = _check_record(rec, b["it"].pool[0])
    nfg, nbg, Fq, Bq = rec["counts"]
    assert rec["seed"] == 3 and S > 0 and Fq >= 4 and Fq <= 16 and S <= 64      # (the four ground-truth boxes are foreground)
    assert int(rec["R"].numpy()[0]) > 0 and np.any(rec["src"].numpy()[:S] >= 4)  # the scan delivered picks, and some were drawn
    assert b["stats"]["rois"] == [rec["counts"]]
    # the anchor nets' part of the step is the plain step's, bit for bit
    gr = _groups(b["model"], b["g"])
    hl, hh = gr["heads"]; cl, ch = gr["cnet"]
    assert same_bits(a["g"][hl:hh], b["g"][hl:hh])
    assert a["stats"]["pcls"] == b["stats"]["pcls"] and a["stats"]["preg"] == b["stats"]["preg"]
    assert np.all(np.isfinite(b["g"])) and np.any(b["g"][cl:ch]) and not same_bits(a["g"][cl:ch], b["g"][cl:ch])
    # one launch more in the classes of scan, selection, NMS; the sampler is counted under rpn (scan: 2 launches)
    names = F._lib.KC_NAMES
    assert lb[names.index("rpn")] > la[names.index("rpn")] and lb[names.index("topk")] > 0 and lb[names.index("nms")] > 0
    # dreg's divisor is F, dcls's is 1: the losses of the sampled rows, from the net's own outputs of this step
    crout, ccout = [t.numpy() for t in b["model"]["cnet"].output]
    ref = cnet_losses_ref(crout[:S], rec["crtarget"].numpy()[:S], ccout[:S], rec["cctarget"].numpy()[:S], S, Fq, rec["bgclass"])
    dreg, dcls = b["stats"]["dreg"][-1], b["stats"]["dcls"][-1]
    assert abs(dreg * Fq - 10.0 * ref["reg_sum"]) <= 1e-6 * 10.0 * ref["reg_sum"]
    assert abs(dcls - ref["cls_mean"]) <= 1e-6 * abs(ref["cls_mean"])


def test_pooled_rows_are_those_of_the_recorded_rects(F, sampled):
    b = sampled[0]
    rec = b["f"].debug["roi_sampling"]
    S = rec["counts"][2] + rec["counts"][3]
    model = b["model"]
    fm = model["pnet"].output[-1]
    fmC, fmH, fmW = fm.shape
    kh, kw, _, _ = F.roi_pooling_settings(model["cfg"])
    loc = F.Localizer(model["pnet"].outnode.children[-1])
    layers = np.array([[l["kW"], l["kH"], l["dW"], l["dH"], l["padW"], l["padH"]] for l in loc.layers], np.int32).reshape(-1, 6)
    wins = F.DeviceTensor.empty((S, 4), np.int32)
    out = F.DeviceTensor.empty((S, fmC * kh * kw), np.float32)
    F._lib.call("frcnn_roi_windows", F.ptr(rec["roi"]), None, S, layers.ctypes.data_as(C.c_void_p), len(layers), fmH, fmW, F.ptr(wins),
                F.stream_ptr())
    F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), fmC, fmH, fmW, F.ptr(wins), S, kh, kw, F.ptr(out), None, F.stream_ptr())
    assert rec["cinput"].shape == (S, fmC * kh * kw)
    assert same_bits(rec["cinput"].numpy(), out.numpy())
    assert wins.numpy().tolist() == F.roi_windows(rec["roi"].numpy()[:S], loc, fmH, fmW).tolist()


def test_roi_align_form(F):
    b = _step(F, PROPOSALS, roi_pooling=dict(method="align"))
    rec = b["f"].debug["roi_sampling"]
    _, S = _check_record(rec, b["it"].pool[0])
    model = b["model"]
    fm = model["pnet"].output[-1]
    fmC, fmH, fmW = fm.shape
    kh, kw, _, g = F.roi_pooling_settings(model["cfg"])
    from frcnn_amd.objective import align_geometry
    inv_sx, inv_sy = align_geometry(F.Localizer(model["pnet"].outnode.children[-1]))
    out = F.DeviceTensor.empty((S, fmC * kh * kw), np.float32)
    F._lib.call("frcnn_roi_align_forward", F.ptr(fm), fmC, fmH, fmW, F.ptr(rec["roi"]), None, S, inv_sx, inv_sy, kh, kw, g, F.ptr(out),
                F.stream_ptr())
    assert same_bits(rec["cinput"].numpy(), out.numpy())
    gr = _groups(model, b["g"])
    assert np.all(np.isfinite(b["g"])) and np.any(b["g"][gr["cnet"][0]:gr["cnet"][1]]) and np.any(b["g"][:gr["heads"][0]])


def test_default_mode_step(F):
    """The configuration users run (deterministic off): the forward pass joins the dense anchor nets, the sparse delta hints are
    set, the losses and the anchor nets' backward pass run on the side stream beside the scan.  Two steps: the sampler's record
    is the restatement's on its recorded inputs, the gradient is finite and every group of it is there."""
    b = _step(F, PROPOSALS, steps=2, det=0)
    rec = b["f"].debug["roi_sampling"]
    _, S = _check_record(rec, b["it"].pool[1])
    assert rec["seed"] == 4 and S > 0 and int(rec["R"].numpy()[0]) > 0 and len(b["stats"]["rois"]) == 2
    assert np.all(np.isfinite(b["g"]))
    for name, (lo, hi) in _groups(b["model"], b["g"]).items():
        assert np.any(b["g"][lo:hi]), name
    assert all(np.isfinite(v) for k in ("pcls", "preg", "dcls", "dreg") for v in b["stats"][k])


def test_threshold_one_leaves_the_ground_truth_alone(F):
    b = _step(F, dict(PROPOSALS, threshold=1.0))
    rec = b["f"].debug["roi_sampling"]
    G = len(b["it"].pool[0]["rois"])
    assert G == 4 and int(rec["R"].numpy()[0]) == 0
    assert rec["counts"] == (G, 0, G, 0)
    assert rec["roi"].numpy()[:G].tobytes() == rec["gt_rect"].tobytes()
    assert not np.any(rec["crtarget"].numpy()[:G]) and rec["cctarget"].numpy()[:G].tolist() == [float(c) for c in rec["gt_class"]]
    assert rec["src"].numpy()[:G].tolist() == list(range(G)) and rec["iou"].numpy()[:G].tolist() == [1.0] * G


def test_an_image_without_boxes_gives_background_rows_only(F):
    def edit(it):
        for x in it.pool:
            x["rois"] = []
    b = _step(F, PROPOSALS, edit=edit)
    rec = b["f"].debug["roi_sampling"]
    nfg, nbg, Fq, Bq = rec["counts"]
    assert (nfg, Fq) == (0, 0) and Bq == min(nbg, 64) and Bq > 0
    assert rec["bgclass"] == b["model"]["cfg"]["class_count"] + 1
    assert rec["cctarget"].numpy()[:Bq].tolist() == [float(rec["bgclass"])] * Bq and not np.any(rec["crtarget"].numpy()[:Bq])
    assert rec["gt_idx"].numpy()[:Bq].tolist() == [-1] * Bq
    gr = _groups(b["model"], b["g"])
    assert np.all(np.isfinite(b["g"])) and np.any(b["g"][gr["cnet"][0]:gr["cnet"][1]])
    assert np.isnan(b["stats"]["dreg"][-1]) and np.isfinite(b["stats"]["dcls"][-1])     # 0 / 0 regression rows (objective.lua:205)


def test_classification_off_launches_nothing_new(F):
    train = dict(proposal=True, classification=False, frozen_blocks=0)
    a, la = _counted(F, lambda: _step(F, train=train))
    b, lb = _counted(F, lambda: _step(F, PROPOSALS, train=train))
    assert la == lb and same_bits(a["g"], b["g"]) and "roi_sampling" not in b["f"].debug and "rois" not in b["stats"]
    # ... and nothing more is uploaded: the example blob carries no ground-truth table
    blob = lambda r: r["f"].debug["scratch"].bufs["blob"].nbytes
    assert blob(a) == blob(b)


@pytest.mark.parametrize("row", ["2_detector", "4_detector_fixed_trunk"])
def test_staged_rows_keep_their_frozen_slices_zero(F, row):
    train = ROWS[row]
    b = _step(F, PROPOSALS, train=train)
    for name, (lo, hi) in _groups(b["model"], b["g"]).items():
        if _frozen(train, name):
            assert not np.any(b["g"][lo:hi]), "%s: %d non-zero elements in a frozen slice" % (name, int(np.count_nonzero(b["g"][lo:hi])))
        else:
            assert np.any(b["g"][lo:hi]), "%s: a trainable slice with no gradient" % name
    _check_record(b["f"].debug["roi_sampling"], b["it"].pool[0])


def test_two_steps_advance_the_seed_and_an_optimiser_step_runs_clean(F):
    state = dict(learningRate=1e-3, momentum=0.9)
    b = _step(F, PROPOSALS, steps=2, run=lambda f, w: F.sgd(f, w, state))
    rec = b["f"].debug["roi_sampling"]
    assert rec["seed"] == 4 and state["evalCounter"] == 2 and len(b["stats"]["rois"]) == 2
    _check_record(rec, b["it"].pool[1])
    assert np.all(np.isfinite(_host(b["w"]))) and np.all(np.isfinite(b["g"]))
    assert all(np.isfinite(v) for k in ("pcls", "preg", "dcls", "dreg") for v in b["stats"][k])


def _refused(F, rs, edit):
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    model["cfg"]["roi_sampling"] = rs
    if edit is not None:
        edit(it)
    g.fill_(7.0)
    torch.cuda.synchronize()

    def call():
        with pytest.raises(F.FrcnnError):
            f(w)
    _, la = _counted(F, call)
    torch.cuda.synchronize()
    assert sum(la) == 0, "a refused pass launched something"
    assert np.all(_host(g) == 7.0), "a refused pass touched the gradient"


def test_a_refused_batch_is_dropped(F):
    """the batch whose ground truth was refused is not tried again: the next call draws the next batch and runs"""
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    model["cfg"]["roi_sampling"] = PROPOSALS
    del it.pool[0]["rois"]
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        with pytest.raises(F.FrcnnError, match="rois"):
            f(w)
        f(w)                                                # pool[1]
        torch.cuda.synchronize()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    _check_record(f.debug["roi_sampling"], it.pool[1])
    assert len(stats["rois"]) == 1 and np.all(np.isfinite(_host(g)))


def test_refused_before_anything_is_queued(F):
    def no_rois(it):
        for x in it.pool:
            del x["rois"]

    def many(it):
        for x in it.pool:
            x["rois"] = [F.Roi(F.Rect(3.0 * k, 2.0, 3.0 * k + 40.0, 60.0), 1 + k % 20) for k in range(65)]

    def flat(it):
        for x in it.pool:
            x["rois"] = [F.Roi(F.Rect(10.0, 10.0, 10.0, 50.0), 2)]
    _refused(F, PROPOSALS, no_rois)
    _refused(F, PROPOSALS, many)
    _refused(F, PROPOSALS, flat)
    _refused(F, dict(PROPOSALS, batch=0), None)
    _refused(F, dict(source="examples", fg_iou=2.0), None)
    _refused(F, dict(PROPOSALS, colour="red"), None)
