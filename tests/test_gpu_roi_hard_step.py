"""Online hard example mining in the training step (cfg["roi_sampling"].source = "hard") at 225x400 on vgg_small, deterministic
mode, explicit dropout masks -- the set-up of tests/test_gpu_roi_sampling.py.  With batch = 4096 and hard_nms_overlap = 1 every
labelled candidate is selected and the step IS the one of "proposals" without a quota, bit for bit: that pins the ascending-row
order, the untouched seed and running statistics of the scoring pass, and the unchanged path behind the sampler.  At batch = 16
the recorded keys, picks and training tables equal the numpy restatement (tests/roi_hard_ref.py) on the recorded inputs.
post_nms_top_n = 192 everywhere: at most 192 + 64 = 256 candidates, the rows the explicit dropout masks of _step hold."""
import numpy as np
import pytest

import roi_hard_ref as H
from test_gpu_optim import _host, same_bits
from test_gpu_roi_sampling import _check_record, _counted, _step
from test_gpu_stages import _groups

pytestmark = pytest.mark.gpu

TOP = 192
NCAP = TOP + 64
NAMES = tuple(name for name, _, _ in H.TABLE)
ALL_PROPOSALS = dict(source="proposals", batch=4096, fg_fraction=1.0, post_nms_top_n=TOP, seed=3)
ALL_HARD = dict(source="hard", batch=4096, hard_nms_overlap=1.0, post_nms_top_n=TOP, seed=3)
HARD16 = dict(source="hard", batch=16, post_nms_top_n=TOP)
TIGHT16 = dict(HARD16, hard_nms_overlap=0.3)       # below the first NMS's 0.7: rows of the step are suppressed


@pytest.fixture(scope="module")
def plain(F):
    return _step(F)


@pytest.fixture(scope="module")
def hard16(F):
    return _step(F, HARD16)


def check_hard_record(rec, entry):
    """the "all" table is the proposal-target layer's without a quota; keys, picks, counts and training tables are the
    restatement's on the recorded inputs -> (the restatement's selection, S, the loss of every row)"""
    rs, a = rec["settings"], rec["all"]
    nfg, nbg, Fa, Ba = a["counts"]
    N = Fa + Ba
    assert (Fa, Ba) == (nfg, nbg) and a["roi"].shape[0] == rec["r_cap"] + (64 if rs["include_gt"] else 0) <= NCAP
    _check_record(dict(rec, settings=dict(rs, fg_quota=a["roi"].shape[0], batch=a["roi"].shape[0]), **a), entry)
    tab = dict((k, a[k].numpy()[:N]) for k in NAMES)
    crout, ccout = [t.numpy()[:N] for t in rec["score"]] if N else (np.zeros((0, 4), np.float32), np.zeros((0, 2), np.float32))
    box5, loss = H.keys_ref(tab["roi"], crout, tab["crtarget"], ccout, tab["cctarget"], Fa)
    if N:
        assert rec["box5"].numpy()[:N].tobytes() == box5.tobytes() and rec["loss"].numpy()[:N].tobytes() == loss.tobytes()
    want = H.select_ref(box5, loss, Fa, rs["batch"], rs["hard_nms_overlap"], tab)
    F_, Bq, surv, n = rec["hard_counts"]
    assert (F_, Bq, surv, n) == want["counts"] and n == N
    if N:
        assert rec["hard_pick"].numpy()[:surv].tolist() == want["pick"].tolist()
    S = F_ + Bq
    for name in NAMES:      # the training tables: the selected rows of the "all" table, in ascending row order
        assert rec[name].numpy()[:S].tobytes() == want[name].tobytes() == tab[name][want["rows"]].tobytes(), name
    assert rec["loss_sel"].numpy()[:S].tobytes() == loss[want["rows"]].tobytes()
    assert rec["counts"] == (nfg, nbg, F_, Bq)
    return want, S, loss


def test_every_row_selected_is_the_proposals_step_without_a_quota(F):
    a = _step(F, ALL_PROPOSALS)
    b = _step(F, ALL_HARD)
    ra, rb = a["f"].debug["roi_sampling"], b["f"].debug["roi_sampling"]
    nfg, nbg, Fq, Bq = ra["counts"]
    S = Fq + Bq
    assert (Fq, Bq) == (nfg, nbg) and S > 16 and nfg >= 4 and nbg > 0 and S <= NCAP
    assert rb["counts"] == ra["counts"] and rb["hard_counts"] == (nfg, nbg, S, S)
    for name in NAMES:
        assert same_bits(ra[name].numpy()[:S], rb[name].numpy()[:S]), name
    assert same_bits(ra["cinput"].numpy(), rb["cinput"].numpy())
    for k in ("pcls", "preg", "dcls", "dreg", "rois"):
        assert a["stats"][k] == b["stats"][k], k
    assert b["stats"]["hard"] == [(S, S)] and "hard" not in a["stats"]
    assert same_bits(a["bn"], b["bn"]), "the scoring pass touched the running statistics"
    assert same_bits(a["g"], b["g"]), "%d gradient elements differ" % int(np.count_nonzero(a["g"] != b["g"]))
    assert a["model"]["native"].seed == b["model"]["native"].seed
    check_hard_record(rb, b["it"].pool[0])


def test_selection_at_a_batch_of_16(F, hard16, plain):
    b, a = hard16, plain
    rec = b["f"].debug["roi_sampling"]
    want, S, loss = check_hard_record(rec, b["it"].pool[0])
    F_, Bq, surv, N = rec["hard_counts"]
    assert 0 < S <= 16 and N > 16 and surv <= N and S == min(16, surv)
    assert b["stats"]["rois"] == [rec["counts"]] and b["stats"]["hard"] == [(N, surv)]
    sel = loss[want["rows"]].astype(np.float64)
    print("N %d, survivors %d, F %d, Bq %d; mean loss selected %.6g, all %.6g" % (N, surv, F_, Bq, sel.mean(), loss.astype(np.float64).mean()))
    assert np.all(np.isfinite(loss)) and sel.mean() >= loss.astype(np.float64).mean()
    # the anchor nets' part of the step is the plain step's, bit for bit
    gr = _groups(b["model"], b["g"])
    hl, hh = gr["heads"]; cl, ch = gr["cnet"]
    assert same_bits(a["g"][hl:hh], b["g"][hl:hh])
    assert a["stats"]["pcls"] == b["stats"]["pcls"] and a["stats"]["preg"] == b["stats"]["preg"]
    assert np.all(np.isfinite(b["g"][cl:ch])) and np.any(b["g"][cl:ch])
    assert rec["cinput"].shape[0] == S


def test_roi_align_form(F):
    b = _step(F, TIGHT16, roi_pooling=dict(method="align"))
    rec = b["f"].debug["roi_sampling"]
    _, S, _ = check_hard_record(rec, b["it"].pool[0])
    print("RoIAlign, overlap 0.3: (F, Bq, survivors, N) = %r" % (rec["hard_counts"],))
    gr = _groups(b["model"], b["g"])
    assert 0 < S <= 16 and np.all(np.isfinite(b["g"])) and np.any(b["g"][gr["cnet"][0]:gr["cnet"][1]]) and np.any(b["g"][:gr["heads"][0]])


def test_an_image_without_boxes_gives_background_rows_only(F):
    def edit(it):
        for x in it.pool:
            x["rois"] = []
    b = _step(F, TIGHT16, edit=edit)
    rec = b["f"].debug["roi_sampling"]
    _, S, _ = check_hard_record(rec, b["it"].pool[0])
    nfg, nbg, F_, Bq = rec["counts"]
    assert (nfg, F_) == (0, 0) and 0 < Bq <= 16 and nbg >= Bq
    assert rec["cctarget"].numpy()[:Bq].tolist() == [float(rec["bgclass"])] * Bq and rec["gt_idx"].numpy()[:Bq].tolist() == [-1] * Bq
    gr = _groups(b["model"], b["g"])
    assert np.all(np.isfinite(b["g"])) and np.any(b["g"][gr["cnet"][0]:gr["cnet"][1]])
    assert np.isnan(b["stats"]["dreg"][-1]) and np.isfinite(b["stats"]["dcls"][-1])


def test_classification_off_launches_nothing_new(F):
    train = dict(proposal=True, classification=False, frozen_blocks=0)
    a, la = _counted(F, lambda: _step(F, train=train))
    b, lb = _counted(F, lambda: _step(F, HARD16, train=train))
    assert la == lb and same_bits(a["g"], b["g"]) and "roi_sampling" not in b["f"].debug
    assert "rois" not in b["stats"] and "hard" not in b["stats"]


def test_two_steps_and_an_optimiser_step_run_clean(F):
    state_p, state_h = dict(learningRate=1e-3, momentum=0.9), dict(learningRate=1e-3, momentum=0.9)
    a = _step(F, dict(HARD16, source="proposals"), steps=2, run=lambda f, w: F.sgd(f, w, state_p))
    b = _step(F, TIGHT16, steps=2, run=lambda f, w: F.sgd(f, w, state_h))
    rec = b["f"].debug["roi_sampling"]
    assert state_h["evalCounter"] == 2 and len(b["stats"]["rois"]) == len(b["stats"]["hard"]) == 2
    assert b["model"]["native"].seed == a["model"]["native"].seed, "the scoring pass advanced the seed"
    check_hard_record(rec, b["it"].pool[1])
    assert np.all(np.isfinite(_host(b["w"]))) and np.all(np.isfinite(b["g"]))
    assert all(np.isfinite(v) for k in ("pcls", "preg", "dcls", "dreg") for v in b["stats"][k])
