"""Staged training (cfg["train"]: proposal / classification / frozen_blocks, Faster R-CNN's 4-step alternating training) on
the device: frozen slices of the gradient stay exactly zero, trainable slices hold the enabled stages' gradient, the library
queues no launch for frozen parts, and the optimisers leave frozen weights and state bit-unchanged."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_optim import (MAIN_NAG, MAIN_SGD, _host, _masks, nag_scalars, ref_lookahead, ref_nag, ref_sgd, same_bits,
                            sgd_scalars)

pytestmark = pytest.mark.gpu

NB = 4   # vgg_small's backbone blocks
ROWS = {   # the paper's four steps, plus two frozen blocks with both stages on
    "1_rpn": dict(proposal=True, classification=False, frozen_blocks=0),
    "2_detector": dict(proposal=False, classification=True, frozen_blocks=0),
    "3_rpn_fixed_trunk": dict(proposal=True, classification=False, frozen_blocks=NB),
    "4_detector_fixed_trunk": dict(proposal=False, classification=True, frozen_blocks=NB),
    "frozen_2": dict(proposal=True, classification=True, frozen_blocks=2),
}


def _setup(F, H, W, seed=11):
    model = F.vgg_small(dict(F.duplo_cfg))
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=seed)
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    f = F.create_objective(model, w, g, it, stats)
    return model, w, g, it, f, stats


def _groups(model, g):
    """name -> [lo, hi) of the parameter groups"""
    pnet = model["pnet"]
    out = {"block%d" % (b + 1): pnet.block_param_range(b) for b in range(NB)}
    out["heads"] = pnet.heads_param_range()
    out["cnet"] = (int(model["native"].pnet_params), int(model["native"].total_params))
    return out


def _frozen(train, name):
    if name == "heads":
        return not train["proposal"]
    if name == "cnet":
        return not train["classification"]
    return int(name[5:]) <= train["frozen_blocks"]


def _step(F, train, H=225, W=400, det=1, steps=1):
    """one (or more) lossAndGradient call(s) with explicit dropout masks -> (gradient, stats, bn running stats, model)"""
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    if train is not None:
        model["cfg"]["train"] = dict(train)
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", det)
    try:
        for k in range(steps):
            _masks(F, model, it, k, H, W, rng)
            f(w)
        torch.cuda.synchronize()
        bn = model["native"].bn_running.cpu().numpy().copy()
        return _host(g).copy(), stats, bn, model
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_frozen_slices_are_exactly_zero(F, row, det):
    """one step: every frozen group's slice of the gradient is exactly zero, every trainable group's is not (the sparse anchor-net
    path in default mode, the dense one in deterministic mode)"""
    train = ROWS[row]
    g, stats, _, model = _step(F, train, det=det)
    for name, (lo, hi) in _groups(model, g).items():
        if _frozen(train, name):
            assert not np.any(g[lo:hi]), "%s: %d non-zero elements in a frozen slice" % (name, int(np.count_nonzero(g[lo:hi])))
        else:
            assert np.any(g[lo:hi]), "%s: a trainable slice with no gradient" % name


def test_frozen_slices_at_450x800(F):
    train = dict(proposal=True, classification=True, frozen_blocks=3)
    g, _, _, model = _step(F, train, H=450, W=800, det=0)
    for name, (lo, hi) in _groups(model, g).items():
        assert np.any(g[lo:hi]) != _frozen(train, name), name


def test_default_settings_equal_no_train_key(F):
    """the default table gives the gradient of a configuration without `train`, bit for bit (deterministic mode), with the same
    launches per kernel class"""
    nk = len(F._lib.KC_NAMES)

    def counted(train):
        la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
        F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
        try:
            g, stats, bn, _ = _step(F, train)
        finally:
            F._lib.call("frcnn_prof_enable", 0)
            F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        return g, stats, bn, list(la)
    a = counted(None)
    b = counted(dict(proposal=True, classification=True, frozen_blocks=0))
    assert same_bits(a[0], b[0])
    assert a[1] == b[1] and same_bits(a[2], b[2])
    assert a[3] == b[3], "launches per class differ: %r vs %r" % (a[3], b[3])


@pytest.mark.parametrize("fb", [1, 2, 3])
def test_frozen_blocks_leave_the_trainable_slices_as_unstaged(F, fb):
    """frozen_blocks = k with both stages on: the trainable slices are the unstaged step's, bit for bit (deterministic mode) --
    the backbone chain is cut below them, nothing they depend on"""
    full, _, _, model = _step(F, None)
    g, _, _, _ = _step(F, dict(proposal=True, classification=True, frozen_blocks=fb))
    lo = model["pnet"].block_param_range(fb)[0]
    assert same_bits(g[lo:], full[lo:])
    assert not np.any(g[:lo])


def test_stages_off_split_the_unstaged_gradient(F):
    """proposal = false keeps the classification net's slice, classification = false the anchor nets' slice, bit for bit; the
    backbone receives the enabled stage's part only, so the two parts add up to the unstaged gradient"""
    full, sf, bnf, model = _step(F, None)
    rpn, sr, bnr, _ = _step(F, dict(proposal=True, classification=False))
    det, sd, _, _ = _step(F, dict(proposal=False, classification=True))
    gr = _groups(model, full)
    hl, hh = gr["heads"]; cl, ch = gr["cnet"]
    assert same_bits(rpn[hl:hh], full[hl:hh]) and same_bits(det[cl:ch], full[cl:ch])
    assert not np.any(rpn[cl:ch]) and not np.any(det[hl:hh])
    both = rpn[:hl].astype(np.float64) + det[:hl]
    ref = full[:hl].astype(np.float64)
    assert np.linalg.norm(both - ref) <= 1e-5 * np.linalg.norm(ref)
    assert np.linalg.norm(rpn[:hl]) > 1e-3 * np.linalg.norm(ref) and np.linalg.norm(det[:hl]) > 1e-3 * np.linalg.norm(ref)
    # statistics: the anchor losses are the unstaged step's; the detector's are NaN without its stage, BN statistics untouched
    assert sr["pcls"] == sf["pcls"] and sr["preg"] == sf["preg"]
    assert sd["pcls"] == sf["pcls"] and sd["preg"] == sf["preg"] and sd["dcls"] == sf["dcls"] and sd["dreg"] == sf["dreg"]
    assert np.isnan(sr["dcls"][0]) and np.isnan(sr["dreg"][0])
    bn0 = np.concatenate([np.zeros(1024, np.float32), np.ones(1024, np.float32)])
    assert same_bits(bnr, bn0) and not same_bits(bnf, bn0)


def test_the_rng_stream_is_the_unstaged_one(F):
    """a step without the detector stage draws what the unstaged step draws: the next step's anchor losses agree (the
    seed-drawn dropout masks of the second step's backbone are the same)"""
    import torch
    res = []
    for train in (None, dict(proposal=True, classification=False)):
        model, w, g, it, f, stats = _setup(F, 225, 400)
        if train is not None:
            model["cfg"]["train"] = train
        F._lib.call("frcnn_set_option", b"deterministic", 1)
        try:
            f(w); f(w)
            torch.cuda.synchronize()
        finally:
            F._lib.call("frcnn_set_option", b"deterministic", 0)
        res.append((stats["pcls"], stats["preg"]))
    assert res[0] == res[1]


def _profile(F, train, forward_half=False):
    """launches per kernel class of the second step (default mode); forward_half: of an unstaged step whose pnet:backward
    (objective.lua:189) is left out -- the forward pass, the anchor losses and the detector stage"""
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    model, w, g, it, f, stats = _setup(F, 225, 400)
    model["cfg"]["train"] = train
    f(w)   # (shapes, workspaces)
    import torch
    torch.cuda.synchronize()
    if forward_half:
        model["pnet"].backward = lambda img, deltas: None
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        f(w)
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return {n: la[i] for i, n in enumerate(F._lib.KC_NAMES)}


def test_work_is_skipped(F):
    """default sparse_heads: a frozen trunk queues no backbone weight-gradient launch, and exactly the conv_x3 launches of the
    step's forward half (no backbone input gradient); without the detector stage no ROI launch runs"""
    full = _profile(F, dict(proposal=True, classification=True, frozen_blocks=0))
    half = _profile(F, dict(proposal=True, classification=True, frozen_blocks=0), forward_half=True)
    trunk = _profile(F, dict(proposal=True, classification=True, frozen_blocks=NB))
    rpn = _profile(F, dict(proposal=True, classification=False, frozen_blocks=0))
    assert full["conv_wgradx"] + full["conv_wgrad_k3"] > 0 and full["roi"] > 0
    assert trunk["conv_wgradx"] == 0 and trunk["conv_wgrad_k3"] == 0
    assert 0 < half["conv_x3"] < full["conv_x3"]
    assert trunk["conv_x3"] == half["conv_x3"], (trunk["conv_x3"], half["conv_x3"])
    assert rpn["roi"] == 0


def test_errors(F):
    model, w, g, it, f, stats = _setup(F, 225, 400)
    for bad in (dict(proposal=False, classification=False), dict(frozen_blocks=NB + 1), dict(frozen_blocks=-1),
                dict(frozen=1), dict(proposal=1)):
        model["cfg"]["train"] = bad
        with pytest.raises(F.FrcnnError):
            f(w)
    with pytest.raises(F.FrcnnError):
        F._lib.call("frcnn_model_set_trainable", model["native"].h, NB + 1, 1, 1)
    with pytest.raises(F.FrcnnError):
        F._lib.call("frcnn_model_set_trainable", model["native"].h, 0, 0, 0)
    fb, hd, cn = C.c_int(), C.c_int(), C.c_int()
    F._lib.call("frcnn_model_get_trainable", model["native"].h, C.byref(fb), C.byref(hd), C.byref(cn))
    assert (fb.value, hd.value, cn.value) == (0, 1, 1)


SWITCH = [dict(proposal=True, classification=False, frozen_blocks=1), dict(proposal=False, classification=True, frozen_blocks=NB),
          dict(proposal=True, classification=True, frozen_blocks=0)]


def _opt_run(F, kind, mode, H=225, W=400):
    """three steps through a stage switch: mode 'fused' / 'eager' / 'unfused' (f(w), then the numpy restatement on the
    trainable slices only) -> per step (weights, state vector)"""
    import torch
    model, w, g, it, f, stats = _setup(F, H, W)
    cfg = dict(rmsprop=dict(learningRate=1e-4, alpha=0.9), sgd=dict(MAIN_SGD), nag=dict(MAIN_NAG, weightDecay=5e-4))[kind]
    if mode != "unfused":
        cfg["eager"] = mode == "eager"
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    out = []
    x_ref = v_ref = None
    try:
        for k, train in enumerate(SWITCH):
            model["cfg"]["train"] = train
            _masks(F, model, it, k, H, W, rng)
            if mode != "unfused":
                getattr(F, kind)(f, w, cfg)
                torch.cuda.synchronize()
                st = cfg["m"] if kind == "rmsprop" else cfg["dfdx"]
                out.append((w.cpu().numpy().copy(), st.cpu().numpy().copy()))
                continue
            ranges = f.trainable_ranges() or [(0, w.numel())]
            if x_ref is None:
                x_ref = w.cpu().numpy().copy()
                v_ref = np.zeros_like(x_ref)
            if kind == "nag" and k > 0:
                for lo, hi in ranges:
                    x_ref[lo:hi] = ref_lookahead(x_ref[lo:hi], v_ref[lo:hi], cfg["momentum"])
                w.copy_(torch.from_numpy(x_ref))
            _, grad = f(w)
            gh = _host(grad)
            for lo, hi in ranges:
                if kind == "rmsprop":
                    f32 = np.float32
                    gs = gh[lo:hi]
                    v_ref[lo:hi] = f32(cfg["alpha"]) * v_ref[lo:hi] + (f32(1) - f32(cfg["alpha"])) * (gs * gs)
                    x_ref[lo:hi] = x_ref[lo:hi] - f32(cfg["learningRate"]) * gs / (np.sqrt(v_ref[lo:hi]) + f32(1e-8))
                elif kind == "sgd":
                    x_ref[lo:hi], _, v_ref[lo:hi] = ref_sgd(x_ref[lo:hi], gh[lo:hi], v_ref[lo:hi], None, sgd_scalars(cfg, k), k == 0)
                else:
                    x_ref[lo:hi], _, v_ref[lo:hi] = ref_nag(x_ref[lo:hi], gh[lo:hi], v_ref[lo:hi], None, nag_scalars(cfg, k), k == 0)
            w.copy_(torch.from_numpy(x_ref))
            torch.cuda.synchronize()
            out.append((x_ref.copy(), v_ref.copy()))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
    return out, _groups(model, g)


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_optimisers_leave_frozen_weights_and_state_alone(F, kind):
    """over a stage switch: what a step freezes keeps its weights and optimiser state bit for bit (a state that did not exist
    before stays 0); eager on == eager off; sgd / nag equal the numpy restatement applied to the trainable slices"""
    fused, groups = _opt_run(F, kind, "fused")
    eager, _ = _opt_run(F, kind, "eager")
    for k, (a, b) in enumerate(zip(fused, eager)):
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), "eager differs from fused after step %d" % k
    model_w0 = _setup(F, 225, 400)[1].cpu().numpy()
    prev_w, prev_s = model_w0, np.zeros_like(model_w0)
    for k, (train, (wk, sk)) in enumerate(zip(SWITCH, fused)):
        for name, (lo, hi) in groups.items():
            if _frozen(train, name):
                assert same_bits(wk[lo:hi], prev_w[lo:hi]), "step %d changed frozen weights of %s" % (k, name)
                assert same_bits(sk[lo:hi], prev_s[lo:hi]), "step %d changed frozen optimiser state of %s" % (k, name)
            else:
                assert not same_bits(wk[lo:hi], prev_w[lo:hi]), "step %d left trainable %s alone" % (k, name)
        prev_w, prev_s = wk, sk
    ref, _ = _opt_run(F, kind, "unfused")
    for k, (a, b) in enumerate(zip(fused, ref)):
        if kind == "rmsprop":   # (m: products and sums, bit for bit; x also divides by a square root: within one ulp)
            ulps = np.abs(a[0].view(np.int32).astype(np.int64) - b[0].view(np.int32))
            assert ulps.max() <= 1, "weights differ from the restatement after step %d (%d ulp)" % (k, int(ulps.max()))
        else:
            assert same_bits(a[0], b[0]), "weights differ from the restatement after step %d" % k
        assert same_bits(a[1], b[1]), "state differs from the restatement after step %d" % k


# ---------------------------------------------------------------- the default mode (sparse anchor nets, fused activations,
# the classification net's weight gradients on their own stream), at the bars of SURVEY 8d: per parameter tensor 1e-3 relative L2
def _tensor_errors(model, got, want, lo=0, hi=None):
    """(offset, relative L2 error) of every parameter tensor inside [lo, hi) with a non-zero reference"""
    hi = len(want) if hi is None else hi
    out = []
    for off, cnt, kind, aux in model["native"].param_table:
        off, cnt = int(off), int(cnt)
        if off < lo or off + cnt > hi:
            continue
        r = want[off:off + cnt].astype(np.float64)
        nr = np.linalg.norm(r)
        if nr > 0:
            out.append((off, np.linalg.norm(got[off:off + cnt] - r) / nr))
    return out


def _assert_tensors(model, got, want, lo=0, hi=None, tol=1e-3, what=""):
    errs = _tensor_errors(model, got, want, lo, hi)
    assert errs, what
    worst = max(errs, key=lambda e: e[1])
    assert worst[1] < tol, "%s: tensor at %d off by %.2e (relative L2)" % (what, worst[0], worst[1])


@pytest.mark.parametrize("fb", [1, 2, 3])
def test_frozen_blocks_default_mode_match_the_unstaged_step(F, fb):
    """frozen_blocks = k, both stages on, default mode: every trainable tensor is the unstaged step's within 1e-3; k = 3 splits
    the sparse anchor nets (net 1 reads block 3, nets 2-4 block 4)"""
    full, _, _, model = _step(F, None, det=0)
    g, _, _, _ = _step(F, dict(proposal=True, classification=True, frozen_blocks=fb), det=0)
    lo = model["pnet"].block_param_range(fb)[0]
    assert not np.any(g[:lo])
    _assert_tensors(model, g, full, lo, what="frozen_blocks=%d" % fb)


def test_stages_off_default_mode_split_the_unstaged_step(F):
    """default mode: the anchor nets' tensors without the detector stage and the classification net's without the RPN stage are
    the unstaged step's within 1e-3; each backbone tensor of the two parts adds up to the unstaged one within 1e-3"""
    full, _, _, model = _step(F, None, det=0)
    rpn, _, _, _ = _step(F, dict(proposal=True, classification=False), det=0)
    det, _, _, _ = _step(F, dict(proposal=False, classification=True), det=0)
    gr = _groups(model, full)
    hl, hh = gr["heads"]; cl, ch = gr["cnet"]
    _assert_tensors(model, rpn, full, hl, hh, what="anchor nets without the detector stage")
    _assert_tensors(model, det, full, cl, ch, what="classification net without the RPN stage")
    assert not np.any(rpn[cl:ch]) and not np.any(det[hl:hh])
    _assert_tensors(model, rpn.astype(np.float64) + det, full, 0, hl, what="backbone: RPN part + detector part")
    for fb in (3, NB):   # the same with the trunk cut: net 1's input block frozen, and every block frozen
        r, _, _, _ = _step(F, dict(proposal=True, classification=False, frozen_blocks=fb), det=0)
        d, _, _, _ = _step(F, dict(proposal=False, classification=True, frozen_blocks=fb), det=0)
        lo = model["pnet"].block_param_range(fb)[0] if fb < NB else hl
        assert not np.any(r[:lo]) and not np.any(d[:lo]) and not np.any(d[hl:hh]) and not np.any(r[cl:ch])
        _assert_tensors(model, r, rpn, lo, ch, what="RPN stage, frozen_blocks=%d" % fb)
        _assert_tensors(model, d, det, lo, ch, what="detector stage, frozen_blocks=%d" % fb)


@pytest.mark.parametrize("fb", [1, 3])
def test_frozen_blocks_against_the_oracle(F, O, fb):
    """smoke()'s oracle comparison (O.train_image, the device's discrete decisions injected, default mode) with the first fb
    blocks frozen: the trainable slices are the oracle's gradient, the frozen ones zero"""
    import decisions
    from util import oracle_model
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    H, W = 128, 176
    it = F.SyntheticBatchIterator(model, H=H, W=W, images_per_batch=1, pool=1, device_images=False)
    model["pnet"].drop_masks = [np.ones(l["filters"], np.float32) for l in model["layers"]]
    ex = it.pool[0]
    sizes = F.output_map_sizes(model, H, W)
    ex["positive"] = F.clean_examples(ex["positive"], sizes)
    ex["negative"] = F.clean_examples(ex["negative"], sizes)
    R = len(ex["positive"]) + len(ex["negative"])
    cm = [np.ones((R, 1024), np.float32), np.ones((R, 512), np.float32)]
    model["cnet"].drop_masks = cm
    model["cfg"]["train"] = dict(frozen_blocks=fb)
    f = F.create_objective(model, weights, gradient, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    with decisions.CaptureBeforeBackward(F, model, f) as cap:
        _, grad = f(weights)
    om = oracle_model(O, cfg)
    w = weights.cpu().numpy()
    g_want = np.zeros_like(w); acc = np.zeros(8)
    rois = ex["rois"]
    pos_idx = np.array([[a.layer, a.aspect, a.index[1], a.index[2], rois.index(r) + 1] for a, r in ex["positive"]], dtype=np.int32).reshape(-1, 5)
    pos_rect = np.array([[a.minX, a.minY, a.maxX, a.maxY] for a, r in ex["positive"]], dtype=np.float64).reshape(-1, 4)
    neg_idx = np.array([[e[0].layer, e[0].aspect, e[0].index[1], e[0].index[2]] for e in ex["negative"]], dtype=np.int32).reshape(-1, 4)
    neg_rect = np.array([[e[0].minX, e[0].minY, e[0].maxX, e[0].maxY] for e in ex["negative"]], dtype=np.float64).reshape(-1, 4)
    roi_rect = np.array([[r.rect.minX, r.rect.minY, r.rect.maxX, r.rect.maxY] for r in rois], dtype=np.float64)
    roi_cls = np.array([r.class_index for r in rois], dtype=np.int32)
    bn = np.concatenate([np.zeros(1024, np.float32), np.ones(1024, np.float32)])
    with O.decisions(inject=cap.captured[0]):
        O.train_image(om, w, g_want, ex["img"], pos_idx, pos_rect, roi_rect, roi_cls, neg_idx, neg_rect,
                      model["pnet"].drop_masks, cm, bn, acc)
    g_want /= acc[2]
    g = grad.cpu().numpy()
    lo = model["pnet"].block_param_range(fb)[0]
    assert not np.any(g[:lo])
    rel = np.linalg.norm(g[lo:] - g_want[lo:]) / np.linalg.norm(g_want[lo:])
    assert rel < 1e-3, rel
    for b in range(fb, NB):
        blo, bhi = model["pnet"].block_param_range(b)
        rb = np.linalg.norm(g[blo:bhi] - g_want[blo:bhi]) / np.linalg.norm(g_want[blo:bhi])
        assert rb < 1e-3, (b + 1, rb)
