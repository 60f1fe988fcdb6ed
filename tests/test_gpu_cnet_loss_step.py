"""cfg["cnet_loss"] in the training step at 225x400 on vgg_small, deterministic mode, explicit dropout masks -- the set-up of
tests/test_gpu_roi_sampling.py and tests/test_gpu_roi_hard_step.py.  With {} the step is the parent's in its gradient, bit for
bit, with one launch more (the rows' sum); under focal + GIoU the step's own outputs, fed to the numpy restatement
(tests/cnet_loss_ref.py), reproduce the gradients the step used and its statistics, for every source of rows; under "hard" the
recorded keys are the restatement's, and with every row selected the step is the one of "proposals" under the same losses."""
import numpy as np
import pytest

import cnet_loss_ref as L
from test_gpu_optim import _host, same_bits
from test_gpu_roi_hard_step import ALL_HARD, ALL_PROPOSALS, HARD16
from test_gpu_roi_sampling import ABSENT, H, W, _counted
from test_gpu_stages import _setup

pytestmark = pytest.mark.gpu

FOCAL_GIOU = dict(cls="focal", box="giou")
PROPOSALS64 = dict(source="proposals", batch=64, fg_fraction=0.25, seed=3, post_nms_top_n=192)


def _step(F, cl=ABSENT, rs=ABSENT):
    """one lossAndGradient call under cfg.cnet_loss = cl and cfg.roi_sampling = rs (the _step of test_gpu_roi_sampling.py with
    the one more key) -> dict(g, stats, model, f)"""
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    cfg = model["cfg"]
    if cl is not ABSENT:
        cfg["cnet_loss"] = cl
    if rs is not ABSENT:
        cfg["roi_sampling"] = rs
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        model["pnet"].drop_masks = [None] + [(rng.rand(c) > 0.4).astype(np.float32) for c in (128, 256, 384)]
        model["cnet"].drop_masks = [(rng.rand(256, 1024) > 0.5).astype(np.float32), (rng.rand(256, 512) > 0.5).astype(np.float32)]
        f(w)
        torch.cuda.synchronize()
        return dict(g=_host(g).copy(), stats=stats, model=model, f=f)
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None


def _rows(b):
    """the rows the step's losses ran on, as host arrays: the sampler's record, or -- the example rows -- debug["cnet_loss"]"""
    rec = b["f"].debug.get("roi_sampling")
    if rec is not None:
        R, npos = rec["counts"][2] + rec["counts"][3], rec["counts"][2]
    else:
        rec = b["f"].debug["cnet_loss"]
        R, npos = rec["R"], rec["npos"]
    return dict((k, rec[k].numpy()[:R].copy()) for k in ("crout", "ccout", "crtarget", "cctarget", "crdelta", "ccdelta")), R, npos


def _stat_bounds(ref, d, R, npos):
    """-> ((dreg, dcls) of the restatement for one image, their bounds): the rows' error bounds, frcnn_loss_accumulate's stated
    bound, and the roundings of the division by the count"""
    (s0, s1), (b0, b1) = L.accumulate_ref(ref["row_loss"])
    e0 = float(np.sum(d["box_weight"] * ref["err"]["box"] + L.ULP * np.abs(ref["row_loss"][:, 0]))) + b0
    e1 = float(np.sum(ref["err"]["cls"] + L.ULP * np.abs(ref["cls"]))) / R + b1
    with np.errstate(all="ignore"):
        dreg = np.float64(s0) / npos
    return (float(dreg), s1), (e0 / max(npos, 1) + L.ULP * abs(float(dreg)), e1 + L.ULP * abs(s1))


def check_against_restatement(b, d):
    t, R, npos = _rows(b)
    assert R > 8 and 0 < npos < R
    ncls = t["ccout"].shape[1]
    ref = L.loss_ref(t["crout"], t["crtarget"], t["ccout"], t["cctarget"], npos, d, bgclass=ncls)
    assert not t["crout"][npos:].any()                      # the step zeroed the background rows
    fin = np.isfinite(ref["crdelta"]) & np.isfinite(ref["ccdelta"]).all(1, keepdims=True)
    assert fin.all()
    assert np.all(np.abs(t["crdelta"].astype(np.float64) - ref["crdelta"]) <= L.spacing32(ref["crdelta"]) + ref["err"]["crdelta"])
    assert np.all(np.abs(t["ccdelta"].astype(np.float64) - ref["ccdelta"]) <= L.spacing32(ref["ccdelta"]) + ref["err"]["gt"][:, None])
    assert np.any(t["crdelta"][:npos]) and np.any(t["ccdelta"])
    (dreg, dcls), (e0, e1) = _stat_bounds(ref, d, R, npos)
    print("R %d, npos %d: dcls %.9g (ref %.9g, bound %.3g), dreg %.9g (ref %.9g, bound %.3g)"
          % (R, npos, b["stats"]["dcls"][-1], dcls, e1, b["stats"]["dreg"][-1], dreg, e0))
    assert abs(b["stats"]["dcls"][-1] - dcls) <= e1 and abs(b["stats"]["dreg"][-1] - dreg) <= e0
    return ref, t, R, npos


@pytest.fixture(scope="module")
def absent(F):
    return _counted(F, lambda: _step(F))


def test_empty_table_is_the_parent_step_with_one_launch_more(F, absent):
    (a, la), (b, lb) = absent, _counted(F, lambda: _step(F, {}))
    assert same_bits(a["g"], b["g"]), "%d gradient elements differ" % int(np.count_nonzero(a["g"] != b["g"]))
    rpn = F._lib.KC_NAMES.index("rpn")
    assert lb[rpn] == la[rpn] + 1 and [v for k, v in enumerate(lb) if k != rpn] == [v for k, v in enumerate(la) if k != rpn]
    for k in ("pcls", "preg"):
        assert a["stats"][k] == b["stats"][k], k
    # the parent rounds each of its two sums to fp32 once (the box sum before the factor 10); the rows' sum is in fp64
    t, R, npos = _rows(b)
    ref = L.loss_ref(t["crout"], t["crtarget"], t["ccout"], t["cctarget"], npos, L.DEFAULT)
    assert t["crdelta"].tobytes() == ref["crdelta"].tobytes() and t["ccdelta"].tobytes() == ref["ccdelta"].tobytes()
    (dreg, dcls), (e0, e1) = _stat_bounds(ref, L.DEFAULT, R, npos)
    assert abs(b["stats"]["dcls"][-1] - dcls) <= e1 and abs(b["stats"]["dreg"][-1] - dreg) <= e0
    pc, pr = a["stats"]["dcls"][-1], a["stats"]["dreg"][-1]
    assert abs(pc - dcls) <= float(np.spacing(np.float32(abs(pc)))) + e1
    assert abs(pr - dreg) <= 10.0 * float(np.spacing(np.float32(abs(pr) * npos / 10.0))) / npos + e0


@pytest.mark.parametrize("rs", [ABSENT, PROPOSALS64, HARD16], ids=["examples", "proposals", "hard"])
def test_focal_and_giou_against_the_restatement(F, absent, rs):
    d = L.desc(**FOCAL_GIOU)
    b = _step(F, dict(FOCAL_GIOU), rs)
    ref, t, R, npos = check_against_restatement(b, d)
    a = absent[0]
    assert not same_bits(a["g"], b["g"])
    assert a["stats"]["pcls"] == b["stats"]["pcls"] and a["stats"]["preg"] == b["stats"]["preg"]     # the anchor nets' losses stay
    if rs is HARD16:
        # the keys that ranked the candidates are this loss on the scoring pass's outputs
        rec = b["f"].debug["roi_sampling"]
        al = rec["all"]
        nfg, nbg, Fa, Ba = al["counts"]
        N = Fa + Ba
        crout, ccout = [x.numpy()[:N] for x in rec["score"]]
        tab = dict((k, al[k].numpy()[:N]) for k in ("roi", "crtarget", "cctarget"))
        want = L.loss_ref(crout, tab["crtarget"], ccout, tab["cctarget"], Fa, d, bgclass=ccout.shape[1], roi=tab["roi"], train=False)
        tol = L.spacing32(want["key"]) + d["box_weight"] * want["err"]["box"] + want["err"]["cls"] \
            + L.ULP * (np.abs(want["cls"]) + np.abs(want["row_loss"][:, 0]))
        loss, box5 = rec["loss"].numpy()[:N], rec["box5"].numpy()[:N]
        assert N > 16 and np.all(np.isfinite(want["key"])) and np.all(np.abs(loss.astype(np.float64) - want["key"]) <= tol)
        assert box5[:, :4].tobytes() == want["box5"][:, :4].tobytes() and box5[:, 4].tobytes() == loss.tobytes()
        assert rec["hard_counts"][3] == N and 0 < R <= 16


def test_every_row_selected_is_the_proposals_step_under_the_same_losses(F):
    a = _step(F, dict(FOCAL_GIOU), ALL_PROPOSALS)
    b = _step(F, dict(FOCAL_GIOU), ALL_HARD)
    ra, rb = a["f"].debug["roi_sampling"], b["f"].debug["roi_sampling"]
    S = ra["counts"][2] + ra["counts"][3]
    assert rb["counts"] == ra["counts"] and rb["hard_counts"] == (ra["counts"][0], ra["counts"][1], S, S) and S > 16
    for k in ("pcls", "preg", "dcls", "dreg", "rois"):
        assert a["stats"][k] == b["stats"][k], k
    assert same_bits(a["g"], b["g"]), "%d gradient elements differ" % int(np.count_nonzero(a["g"] != b["g"]))


def test_a_bad_table_is_refused_before_the_step(F):
    model, w, g, it, f, stats = _setup(F, H, W)
    model["cfg"]["cnet_loss"] = dict(cls="focal", label_smoothing=0.1)
    with pytest.raises(F.FrcnnError, match="cnet_loss"):
        f(w)


def test_validation_losses_report_the_same_loss(F):
    from test_gpu_eval import _Val
    cfg = dict(F.duplo_cfg); cfg["cnet_loss"] = dict(FOCAL_GIOU, alpha=0.25)
    d = L.desc(alpha=0.25, **FOCAL_GIOU)
    model = F.vgg_small(cfg)
    F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=3)
    items = [dict(img=F.synthetic_image(128, 176, 40 + k), rois=F.synthetic_rois(cfg, 176, 128, 3, 7, 40 + k)) for k in range(2)]
    rows = []
    res = F.validation_losses(model, _Val(F.Anchors(model["pnet"], cfg["scales"]), items), 2, debug=rows)
    assert len(rows) >= 1 and res["positives"] > 0
    creg = ccls = e_reg = e_cls = 0.0
    for t in rows:
        ref = L.loss_ref(t["crout"], t["crtarget"], t["ccout"], t["cctarget"], t["npos"], d, bgclass=t["ccout"].shape[1])
        (s0, s1), (b0, b1) = L.accumulate_ref(ref["row_loss"])
        creg += s0; ccls += s1
        e_reg += float(np.sum(d["box_weight"] * ref["err"]["box"] + L.ULP * np.abs(ref["row_loss"][:, 0]))) + b0 + L.ULP * abs(creg)
        e_cls += float(np.sum(ref["err"]["cls"] + L.ULP * np.abs(ref["cls"]))) / t["R"] + b1 + L.ULP * abs(ccls)
    assert abs(res["dcls"] - ccls / res["images"]) <= e_cls / res["images"] + L.ULP * abs(res["dcls"])
    assert abs(res["dreg"] - creg / res["positives"]) <= e_reg / res["positives"] + L.ULP * abs(res["dreg"])
    plain = dict(cfg); del plain["cnet_loss"]
    model["cfg"] = plain
    base = F.validation_losses(model, _Val(F.Anchors(model["pnet"], cfg["scales"]), items), 2)
    assert base["dcls"] != res["dcls"] and base["dreg"] != res["dreg"] and base["pcls"] == res["pcls"]
