"""The classification net (csrc/cnet.hip, net.cpp frcnn_cnet_forward / frcnn_cnet_backward) across row counts, layer
tables and class counts (tests/cnet_plan.py: the tables and the branch each entry exists to reach), against the oracle
with the device's PReLU branches injected, at the bars of test_gpu_widths.py::test_cnet_rows; evaluate mode, the dropout
masks drawn on the device against a numpy restatement of the draw, and deterministic mode.

Conditioning is a precondition of every training case, not a tolerance: the oracle itself runs twice, on x and on
x * (1 + 1e-6 randn), and must move by at most a tenth of the bar (see cnet_plan.SEED_OVERRIDES)."""
import ctypes as C

import numpy as np
import pytest

import cnet_plan as CP
import decisions
import width_plan as WP
from test_gpu_model import _compare_gradient
from util import assert_close, rel_close

pytestmark = pytest.mark.gpu

PROBE_BAR = 1e-5   # a tenth of the 1e-4 bar on outputs and gradInput


# ---- the oracle's half (no device needed: the seeds of cnet_plan.py were chosen by running it on the CPU) ----------------
def oracle_setup(O, cfg0, key):
    table, L, cc = key
    cfg = dict(cfg0)
    cfg["class_count"] = cc
    layers, anchor_nets, class_layers = WP.layers_of(CP.BACKBONE + [L]), WP.heads_of(CP.HEADS), CP.cls_of(table)
    return cfg, layers, anchor_nets, class_layers, O.make_model(layers, anchor_nets, class_layers, cfg)


def bn_initial(key):
    """running mean 0, running variance 1 per batch-normalised layer (utilities.py combine_and_flatten_parameters)"""
    return np.concatenate([np.r_[np.zeros(n), np.ones(n)] for n, bn, p in CP.TABLES[key[0]] if bn] or [np.zeros(0)]).astype(np.float32)


def oracle_pass(O, om, w, bn, x, masks, gb, gc, training=True, inject=None):
    """-> dict(bbox, cls, gx, g, bn, own): one forward + backward of the oracle; bn (updated in place by a training pass) is
    copied first.  inject: the PReLU branches to take as given."""
    bn = bn.copy()
    g = np.zeros_like(w)
    rec = dict(cnet_pos=[np.zeros((x.shape[0], l), np.uint8) for l in [om.cls_n[i] for i in range(om.ncls)]])
    own = decisions.blank_like(rec)
    with O.decisions(inject=inject, record=own):
        wb, wc, st = O.cnet_forward(om, w, x, training, masks if training else None, bn)
        gx = O.cnet_backward(om, w, st, gb, gc, g, x.shape[1])
    return dict(bbox=wb, cls=wc, gx=gx, g=g, bn=bn, own=own)


def oracle_probe(O, om, w, key, R, seed):
    """-> (the largest movement of bbox, log-probabilities and gradInput in assert_close's measure when the input moves by
    a relative 1e-6, the case's inputs)"""
    c = CP.inputs(key, R, seed)
    bn0 = bn_initial(key)
    a = oracle_pass(O, om, w, bn0, c["x"], c["masks"], c["gb"], c["gc"])
    b = oracle_pass(O, om, w, bn0, c["x2"], c["masks"], c["gb"], c["gc"])
    moved = max(rel_close(b[k], a[k])[1] for k in ("bbox", "cls", "gx"))
    return moved, c


def layout(key, pn):
    """offsets in the flat parameter vector (orc_model.c): per hidden layer W [n][in], b, (gamma, beta), slope; then the bbox
    head and the class head -> ([dict(W, b, gamma, beta, a, n, fin)], dict(Wb, bb, Wc, bc, nf))"""
    table, L, cc = key
    off, fin, out = pn, CP.ROI_CELLS * L, []
    for n, bn, p in CP.TABLES[table]:
        d = dict(n=n, fin=fin, W=off, b=off + fin * n)
        off += fin * n + n
        if bn:
            d.update(gamma=off, beta=off + n)
            off += 2 * n
        d["a"] = off
        off += 1
        out.append(d)
        fin = n
    nc = cc + 1
    heads = dict(nf=fin, Wb=off, bb=off + 4 * fin, Wc=off + 4 * fin + 4, bc=off + 4 * fin + 4 + nc * fin)
    return out, heads


def linear_output_gradients(key, pn, w, c, pos):
    """The gradient at the output of every hidden Linear, [R][n] per layer, of one training pass in float64 numpy (PReLU
    branches `pos` as given): what the layer's bias gradient sums over the rows."""
    table, L, cc = key
    lay, hd = layout(key, pn)
    w = w.astype(np.float64)
    R = c["x"].shape[0]
    cur, st = c["x"].astype(np.float64), []
    for l, (d, (n, bn, p)) in enumerate(zip(lay, CP.TABLES[table])):
        lin = cur @ w[d["W"]:d["W"] + d["fin"] * n].reshape(n, d["fin"]).T + w[d["b"]:d["b"] + n]
        xhat = inv = None
        pre = lin
        if bn:
            inv = 1.0 / np.sqrt(lin.var(0) + 1e-5)
            xhat = (lin - lin.mean(0)) * inv
            pre = xhat * w[d["gamma"]:d["gamma"] + n] + w[d["beta"]:d["beta"] + n]
        scale = c["masks"][l].astype(np.float64) / (1.0 - p) if p > 0 else 1.0
        cur = np.where(pos[l] > 0, pre, w[d["a"]] * pre) * scale
        st.append((xhat, inv, scale))
    nf, nc = hd["nf"], cc + 1
    Wb, Wc = w[hd["Wb"]:hd["Wb"] + 4 * nf].reshape(4, nf), w[hd["Wc"]:hd["Wc"] + nc * nf].reshape(nc, nf)
    logits = cur @ Wc.T + w[hd["bc"]:hd["bc"] + nc]
    sm = np.exp(logits - logits.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    gc = c["gc"].astype(np.float64)
    g = c["gb"].astype(np.float64) @ Wb + (gc - sm * gc.sum(1, keepdims=True)) @ Wc
    glin = [None] * len(lay)
    for l in range(len(lay) - 1, -1, -1):
        d, (n, bn, p) = lay[l], CP.TABLES[table][l]
        xhat, inv, scale = st[l]
        g = g * scale
        g = np.where(pos[l] > 0, g, w[d["a"]] * g)
        if bn:
            gm = w[d["gamma"]:d["gamma"] + n]
            g = (g - g.mean(0) - xhat * (g * xhat).mean(0)) * gm * inv
        glin[l] = g
        g = g @ w[d["W"]:d["W"] + d["fin"] * n].reshape(n, d["fin"])
    return glin, g


# The bias of a Linear in front of a BatchNormalization has gradient ZERO: the batch normalisation's input gradient sums to
# zero over the rows.  Each side computes it as the sum of R float32 values v, each rounded by up to half an ulp (uniform:
# standard deviation 2^-23 |v| / sqrt(12) at most), so a side's residue over the n columns has norm 2^-23 / sqrt(12) * |v|_F,
# two independent sides sqrt(2) times that; the factor 2 on top covers the spread of that norm and the last-bit differences of
# the summed values themselves.  _compare_gradient's floor for such tensors, 1e-6 sqrt(n), is an absolute number that this
# residue outgrows with sqrt(R) and with the size of the gradient, so for these tensors the bar is the larger of the two.
ROUNDING = 2.0 ** -23 / np.sqrt(12.0)


def zero_bias_bound(glin):
    return 2.0 * np.sqrt(2.0) * ROUNDING * np.linalg.norm(glin)


# ---- the device's half ---------------------------------------------------------------------------------------------------
class _Nets(object):
    """one model per (table, L, class_count), built when its first case runs; the oracle's results per case, shared by the
    modes that run it (they are never written to)"""

    def __init__(self, F, O):
        self.F, self.O, self.models, self.probed, self.wanted, self.trained = F, O, {}, {}, {}, {}

    def get(self, key):
        if key not in self.models:
            F, O = self.F, self.O
            cfg, layers, anchor_nets, class_layers, om = oracle_setup(O, F.duplo_cfg, key)
            model = F.create_model(cfg, layers, anchor_nets, class_layers)
            weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=CP.WEIGHT_SEED)
            nat = model["native"]
            assert O.param_count(om) == (nat.total_params, nat.pnet_params)
            bn0 = nat.bn_running.cpu().numpy().copy() if nat.bn_running is not None else np.zeros(0, np.float32)
            assert np.array_equal(bn0, bn_initial(key))
            self.models[key] = dict(key=key, cfg=cfg, model=model, weights=weights, gradient=gradient, om=om,
                                    w=weights.cpu().numpy().copy(), bn0=bn0)
        return self.models[key]

    def probe(self, key, R):
        """the conditioning probe of a training case, once per case"""
        if (key, R) not in self.probed:
            s = self.get(key)
            self.probed[(key, R)] = oracle_probe(self.O, s["om"], s["w"], key, R, CP.seed_of(key, R))
        moved, c = self.probed[(key, R)]
        print("%s R = %d: the oracle moves by %.2e under a relative 1e-6 of the input" % (CP.model_id(key), R, moved))
        assert moved <= PROBE_BAR, "%s R = %d seed %d is badly conditioned (%.2e): choose another seed in cnet_plan.py" % (
            CP.model_id(key), R, CP.seed_of(key, R), moved)
        return c

    def want(self, tag, s, bn, c, dec, training=True):
        """the oracle with the device's branches injected; the fused / separate / option variants of one case nearly always
        decide alike, and then share one oracle run"""
        k = (tag, training, bn.tobytes(), b"".join(d.tobytes() for d in dec["cnet_pos"]))
        if k not in self.wanted:
            self.wanted[k] = oracle_pass(self.O, s["om"], s["w"], bn, c["x"], c["masks"], c["gb"], c["gc"], training, inject=dec)
        return self.wanted[k]


@pytest.fixture(scope="module")
def nets(F, O):
    return _Nets(F, O)


def _restore(s):
    import torch
    nat = s["model"]["native"]
    s["model"]["cnet"].drop_masks = None
    s["model"]["cnet"].training()
    if nat.bn_running is not None:
        nat.bn_running.copy_(torch.from_numpy(s["bn0"]))


def _bn(s):
    nat = s["model"]["native"]
    return nat.bn_running.cpu().numpy().copy() if nat.bn_running is not None else np.zeros(0, np.float32)


def device_pass(F, s, c, masks, training=True):
    """cnet.forward + cnet.backward -> dict(bbox, cls, gx, g, bn, dec, seed); masks None: drawn on the device"""
    model = s["model"]
    cnet, nat = model["cnet"], model["native"]
    R = c["x"].shape[0]
    if training:
        cnet.training()
    else:
        cnet.evaluate()
    cnet.drop_masks = masks
    x = F.DeviceTensor.from_numpy(c["x"])
    bbox, cls = cnet.forward(x)
    out = dict(bbox=bbox.numpy().copy(), cls=cls.numpy().copy(), seed=nat.seed, bn=_bn(s))
    out["pre"] = [decisions._dev_array(F, nat, 3, i, np.float32, (R, n)) for i, (n, bn, p) in enumerate(CP.TABLES[s["key"][0]])]
    out["dec"] = dict(cnet_pos=[np.ascontiguousarray((p > 0).astype(np.uint8)) for p in out["pre"]])
    s["gradient"].zero_()
    gx = cnet.backward(x, [F.DeviceTensor.from_numpy(c["gb"]), F.DeviceTensor.from_numpy(c["gc"])])
    out["gx"] = gx.numpy().copy()
    cnet.join_backward()
    out["g"] = s["gradient"].cpu().numpy().copy()
    assert all(np.isfinite(out[k]).all() for k in ("bbox", "cls", "gx", "g"))
    return out


def compare(s, c, got, want, what, training=True):
    """test_gpu_widths.py::test_cnet_rows' bars (training=False: an evaluate-mode pass, which writes no running statistics
    and whose batch normalisation does not couple the rows)"""
    nat = s["model"]["native"]
    assert_close(got["bbox"], want["bbox"], 1e-4, what + " bbox")
    assert_close(got["cls"], want["cls"], 1e-4, what + " log-probabilities")
    if training:
        assert_close(got["bn"], want["bn"], 1e-5, what + " bn running statistics")
    if got["dec"]["cnet_pos"]:
        nd, nt = decisions.count_differences(got["dec"], want["own"])["cnet_pos"]
        assert nd <= max(4, 2e-5 * nt), (what, nd, nt)
    assert_close(got["gx"], want["gx"], 1e-4, what + " gradInput")
    g = got["g"].copy()
    if training:
        # the biases in front of a batch normalisation (true gradient zero): see zero_bias_bound; every other tensor, and the
        # elementwise bar of these, through _compare_gradient as it stands
        glin, gx64 = linear_output_gradients(s["key"], nat.pnet_params, s["w"], c, got["dec"]["cnet_pos"])
        assert_close(want["gx"], gx64, 1e-5, what + " (float64 numpy against the oracle) gradInput")
        for d, v, (n, bn, p) in zip(layout(s["key"], nat.pnet_params)[0], glin, CP.TABLES[s["key"][0]]):
            if not bn:
                continue
            a, b = got["g"][d["b"]:d["b"] + n].astype(np.float64), want["g"][d["b"]:d["b"] + n].astype(np.float64)
            bar = max(1e-6 * np.sqrt(n), zero_bias_bound(v))
            print("%s: bias of the %d-wide Linear in front of a batch normalisation: device %.2e oracle %.2e difference %.2e bar %.2e" % (
                what, n, np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(a - b), bar))
            assert np.linalg.norm(b) <= bar and np.linalg.norm(a - b) <= bar, (what, n, np.linalg.norm(a - b), np.linalg.norm(b), bar)
            g[d["b"]:d["b"] + n] = want["g"][d["b"]:d["b"] + n]
    _compare_gradient(nat, g, want["g"], lo=nat.pnet_params, hi=nat.total_params)
    assert not got["g"][:nat.pnet_params].any(), what + ": the classification net wrote the proposal net's gradient"


def _fuse(monkeypatch, fuse):
    if fuse == "separate":
        monkeypatch.setenv("FRCNN_CNET_FUSE", "0")
    else:
        monkeypatch.delenv("FRCNN_CNET_FUSE", raising=False)


def _option(F, name):
    v = C.c_int(-1)
    F._lib.call("frcnn_get_option", name, C.byref(v))
    return v.value


def training_case(F, nets, key, R, what):
    s = nets.get(key)
    c = nets.probe(key, R)
    try:
        got = device_pass(F, s, c, c["masks"])
        want = nets.want((key, R), s, s["bn0"], c, got["dec"])
        compare(s, c, got, want, what)
    finally:
        _restore(s)
    return s, c, got, want


# ---- a. training forward and backward against the oracle -----------------------------------------------------------------
CASE_IDS = ["%s-R%d" % (CP.model_id(k), R) for k, R in CP.cases()]


@pytest.mark.parametrize("fuse", ["fused", "separate"])
@pytest.mark.parametrize("key,R", CP.cases(), ids=CASE_IDS)
def test_training_against_the_oracle(F, nets, monkeypatch, key, R, fuse):
    """explicit dropout masks, the device's PReLU branches injected: outputs and gradInput 1e-4, running statistics 1e-5,
    every gradient tensor of the classification net at _compare_gradient's bars, with the fused launches and with one
    launch per operation (FRCNN_CNET_FUSE=0)."""
    _fuse(monkeypatch, fuse)
    training_case(F, nets, key, R, "%s R = %d %s" % (CP.model_id(key), R, fuse))


@pytest.mark.parametrize("fuse", ["fused", "separate"])
def test_one_row_through_a_batch_normalisation(F, nets, monkeypatch, fuse):
    """R = 1 on `one`: xhat is exactly zero, so the layer's activation is the batch normalisation's bias (given values other
    than the initial zeros here) and nothing of the output gradient passes the batch normalisation, on both sides"""
    import torch
    _fuse(monkeypatch, fuse)
    key, R = ("one", 32, CP.CLASS_COUNT), 1
    s0 = nets.get(key)
    nat = s0["model"]["native"]
    n = CP.TABLES["one"][0][0]
    d = layout(key, nat.pnet_params)[0][0]
    w = s0["w"].copy()
    w[d["beta"]:d["beta"] + n] = np.random.RandomState(7).uniform(-1, 1, n).astype(np.float32)
    s = dict(s0, w=w)
    c = CP.inputs(key, R, CP.seed_of(key, R))
    try:
        s["weights"].copy_(torch.from_numpy(w))
        got = device_pass(F, s, c, c["masks"])
        want = nets.want((key, R, "beta"), s, s["bn0"], c, got["dec"])
        compare(s, c, got, want, "one R = 1 %s" % fuse)
        assert np.array_equal(got["pre"][0], w[None, d["beta"]:d["beta"] + n]) and got["pre"][0].any()
        assert not got["gx"].any() and not want["gx"].any()
    finally:
        s["weights"].copy_(torch.from_numpy(s0["w"]))
        _restore(s0)


ASYNC_CASES = [(k, R) for k, R in CP.cases() if k[0] in CP.ASYNC_TABLES and k[2] == CP.CLASS_COUNT]


@pytest.mark.parametrize("wgrad_async", [0, 1])
@pytest.mark.parametrize("fuse", ["fused", "separate"])
@pytest.mark.parametrize("key,R", ASYNC_CASES, ids=["%s-R%d" % (CP.model_id(k), R) for k, R in ASYNC_CASES])
def test_training_with_the_weight_gradients_on_and_off_the_chain(F, nets, monkeypatch, key, R, fuse, wgrad_async):
    """option cnet_wgrad_async: with it on, a layer's input gradient may reach the layer below as split-K slabs (the gdefer
    condition of frcnn_cnet_backward); with it off every product folds its own."""
    _fuse(monkeypatch, fuse)
    before = _option(F, b"cnet_wgrad_async")
    F._lib.call("frcnn_set_option", b"cnet_wgrad_async", wgrad_async)
    try:
        training_case(F, nets, key, R, "%s R = %d %s cnet_wgrad_async = %d" % (CP.model_id(key), R, fuse, wgrad_async))
    finally:
        F._lib.call("frcnn_set_option", b"cnet_wgrad_async", before)


# ---- b. evaluate mode ----------------------------------------------------------------------------------------------------
TRAIN_ROWS_BEFORE_EVAL = 1025


@pytest.mark.parametrize("fuse", ["fused", "separate"])
@pytest.mark.parametrize("R", CP.EVAL_ROWS)
@pytest.mark.parametrize("table", CP.EVAL_TABLES)
def test_evaluate_mode(F, nets, monkeypatch, table, R, fuse):
    """after one training pass (running statistics updated on both sides): the evaluate-mode forward, and at R <= 1025 its
    backward, against the oracle with the oracle's own updated statistics"""
    _fuse(monkeypatch, fuse)
    key = (table, 32, CP.CLASS_COUNT)
    import torch
    if (key, fuse) not in nets.trained:   # one training pass per (table, mode): the statistics of both sides
        s, c0, got0, want0 = training_case(F, nets, key, TRAIN_ROWS_BEFORE_EVAL, "%s training pass" % table)
        nets.trained[(key, fuse)] = dict(bn=got0["bn"]), dict(bn=want0["bn"])
    got0, want0 = nets.trained[(key, fuse)]
    s = nets.get(key)
    nat = s["model"]["native"]
    c = CP.inputs(key, R, 1000 + R)
    what = "%s evaluate R = %d %s" % (table, R, fuse)
    try:
        nat.bn_running.copy_(torch.from_numpy(got0["bn"]))   # (the device's own statistics of the training pass)
        got = device_pass(F, s, c, None, training=False)
        want = nets.want((key, R, "eval"), s, want0["bn"], c, got["dec"], training=False)
        assert np.array_equal(got["bn"], got0["bn"]), what + ": evaluate mode wrote the running statistics"
        assert_close(got["bbox"], want["bbox"], 1e-4, what + " bbox")
        assert_close(got["cls"], want["cls"], 1e-4, what + " log-probabilities")
        if R in CP.EVAL_BACKWARD_ROWS:
            compare(s, c, got, want, what, training=False)
    finally:
        _restore(s)


# ---- c. masks drawn on the device ----------------------------------------------------------------------------------------
def predicted_masks(table, R, s):
    """the masks cnet.forward draws when native.seed is s after its increment: layer l takes stream s * 977 + l + 17"""
    return [CP.keep_mask(s * 977 + l + 17, R * n, p).reshape(R, n) if p > 0 else None for l, (n, bn, p) in enumerate(CP.TABLES[table])]


DRAW_SEED = 4000   # native.seed before the call (the streams, and with them the guard below, do not depend on the tests that ran before)


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("R", CP.DRAW_ROWS)
@pytest.mark.parametrize("table", CP.DRAW_TABLES)
def test_masks_drawn_on_the_device(F, nets, monkeypatch, table, R, det):
    """drop_masks = None: the masks the kernels draw are the numpy restatement's -- the pass with the predicted masks handed
    in gives the same bits (deterministic mode: the gradient too; default: the gradient within 1e-6 of its norm); the fused
    and the separate launches draw the same streams; two consecutive calls draw different masks."""
    key = (table, 32, CP.CLASS_COUNT)
    s = nets.get(key)
    nat = s["model"]["native"]
    c = CP.inputs(key, R, CP.seed_of(key, R))
    lo = nat.pnet_params
    seed0 = nat.seed
    F._lib.call("frcnn_set_option", b"deterministic", det)
    runs = {}
    try:
        for fuse in ("fused", "separate"):
            _fuse(monkeypatch, fuse)
            nat.seed = DRAW_SEED + R
            drawn = device_pass(F, s, c, None)
            assert drawn["seed"] == DRAW_SEED + R + 1
            _restore(s)
            masks = predicted_masks(table, R, drawn["seed"])
            for l, m in enumerate(masks):
                assert (m is None) == (CP.TABLES[table][l][2] == 0)
                assert m is None or 0.4 <= m.mean() <= 0.6, (l, m.mean())
            given = device_pass(F, s, c, masks)
            _restore(s)
            what = "%s R = %d %s: drawn on the device / predicted masks handed in" % (table, R, fuse)
            for k in ("bbox", "cls", "gx", "bn"):
                assert np.array_equal(drawn[k], given[k]), what + ": " + k
            ga, gb = drawn["g"][lo:].astype(np.float64), given["g"][lo:].astype(np.float64)
            assert np.abs(gb).max() > 0
            if det:
                assert np.array_equal(drawn["g"], given["g"]), what + ": gradient"
            else:
                assert np.linalg.norm(ga - gb) <= 1e-6 * np.linalg.norm(gb), (what, np.linalg.norm(ga - gb) / np.linalg.norm(gb))
            # the next call draws other masks
            nxt = device_pass(F, s, c, None)
            _restore(s)
            assert nxt["seed"] > drawn["seed"]
            other = predicted_masks(table, R, nxt["seed"])
            assert all(m is None or (m != o).mean() > 0.25 for m, o in zip(masks, other))
            assert not np.array_equal(nxt["bbox"], drawn["bbox"]) and not np.array_equal(nxt["gx"], drawn["gx"])
            runs[fuse] = drawn
        a, b = runs["fused"], runs["separate"]   # test_cnet_fused_layers_equal_separate_launches' bars
        for k in ("bbox", "cls", "gx", "bn"):
            assert_close(a[k], b[k], 1e-6, "%s R = %d fused / separate with drawn masks: %s" % (table, R, k))
        ga, gb = a["g"][lo:].astype(np.float64), b["g"][lo:].astype(np.float64)
        assert np.linalg.norm(ga - gb) <= 1e-6 * np.linalg.norm(gb), (table, R, np.linalg.norm(ga - gb) / np.linalg.norm(gb))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        nat.seed = seed0
        _restore(s)


# ---- d. deterministic mode -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", ["fused", "separate"])
@pytest.mark.parametrize("R", CP.DET_ROWS)
@pytest.mark.parametrize("table", CP.DET_TABLES)
def test_deterministic_mode(F, nets, monkeypatch, table, R, fuse):
    """frcnn_set_option("deterministic", 1): the bars of part a against the oracle, and two runs bit-identical"""
    _fuse(monkeypatch, fuse)
    key = (table, 32, CP.CLASS_COUNT)
    assert _option(F, b"deterministic") == 0
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        s, c, first, want = training_case(F, nets, key, R, "%s R = %d %s deterministic" % (table, R, fuse))
        second = device_pass(F, s, c, c["masks"])
        for k in ("bbox", "cls", "gx", "g", "bn"):
            assert np.array_equal(first[k], second[k]), "%s R = %d %s: %s differs between two deterministic runs" % (table, R, fuse, k)
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        _restore(nets.get(key))
