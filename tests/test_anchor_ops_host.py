"""The references of tests/anchor_ops_ref.py checked without a GPU: the geometry against the oracle, the criteria against
torch.nn.functional in float64, the scan order against a literal loop, and the input conditions that tests/test_gpu_anchor_ops.py
relies on, asserted on every problem it runs."""
import math

import numpy as np
import pytest

import anchor_ops_ref as ref
from util import oracle_model

CFG = dict(class_count=16, scales=[32, 64, 128, 256], roi_pooling=dict(kw=6, kh=6))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------ geometry against the oracle
def test_geometry_against_the_oracle(O):
    OA = O.Anchors(oracle_model(O, CFG))
    aw, ah = OA.w_table, OA.h_table
    assert aw.dtype == np.float32 and aw.shape == (4, 3, 200, 2)
    rng = np.random.RandomState(5)
    for _ in range(300):
        l, a, y, x = rng.randint(1, 5), rng.randint(1, 4), rng.randint(1, 201), rng.randint(1, 201)
        an = ref.anchor_get(aw, ah, l, a, y, x)
        assert np.array_equal(np.array(an), OA.get(l, a, y, x))
        w, h = an[2] - an[0], an[3] - an[1]
        roi = (an[0] + rng.uniform(-0.4, 0.4) * w, an[1] + rng.uniform(-0.4, 0.4) * h)
        roi = roi + (roi[0] + w * math.exp(rng.uniform(-0.5, 0.5)), roi[1] + h * math.exp(rng.uniform(-0.5, 0.5)))
        t = np.array(ref.input_to_anchor(an, roi), np.float32)
        assert np.array_equal(bits(t), bits(O.input_to_anchor(an, roi)))
        t = rng.randn(4).astype(np.float32)
        assert np.array_equal(np.array(ref.anchor_to_input(an, t)), O.anchor_to_input(an, t))
    # edge targets: a roi of the anchor's extent at a dyadic offset
    an = (12.25, 40.5, 76.25, 72.5)
    assert ref.input_to_anchor(an, (12.25 - 32.0, 40.5 + 8.0, 12.25 + 32.0, 40.5 + 40.0)) == (-0.5, 0.25, 0.0, 0.0)


def test_scan_ref_rects_against_the_oracle_and_a_literal_loop(O):
    """every match of a scan problem: the rect through the oracle's anchor_to_input on the oracle's Anchors.get, the decision
    through Rect.overlaps, the log-probability through torch's float64 log_softmax"""
    import torch
    c = ref.scan_case("n1287", "random")
    w = c["want"]
    assert w["count"] > 100
    lit = _literal_scan(c)
    assert [list(m[0]) for m in lit] == w["idx"].tolist()
    for i, (idx, p, r) in enumerate(lit):
        l, a, y, x = idx
        t = c["maps"][l - 1][(a - 1) * 6 + 2:(a - 1) * 6 + 6, y - 1, x - 1]
        want = O.anchor_to_input(ref.anchor_get(c["aw"], c["ah"], l, a, y, x), t)
        assert np.all(np.abs(w["rect"][i] - want) <= w["rect_tol"][i])
        assert np.all(np.abs(np.array(r) - want) == 0)       # the literal loop and the oracle share libm
        v = torch.tensor(c["maps"][l - 1][(a - 1) * 6:(a - 1) * 6 + 2, y - 1, x - 1].astype(np.float64))
        lp = float(torch.nn.functional.log_softmax(v, 0)[0])
        assert abs(float(w["p"][i]) - lp) <= 0.5 * w["p_tol"][i] and abs(p - lp) <= 0.5 * w["p_tol"][i]
        assert np.array_equal(bits(w["box"][i]), bits(np.array(want, np.float32))) or np.all(
            np.abs(w["box"][i].astype(np.float64) - want) <= w["box_tol"][i])


def _literal_scan(c):
    """Detector.lua:39-66 as it stands: layer, y, x, aspect; -> [((layer, aspect, y, x), p, rect)]"""
    out = []
    for i in range(1, 5):
        layer = c["maps"][i - 1]
        for y in range(1, layer.shape[1] + 1):
            for x in range(1, layer.shape[2] + 1):
                col = layer[:, y - 1, x - 1]
                for a in range(1, 4):
                    ofs = (a - 1) * 6
                    l0, _, _ = ref.log_softmax2(col[ofs], col[ofs + 1])
                    if math.exp(l0) > ref.THR:
                        an = ref.anchor_get(c["aw"], c["ah"], i, a, y, x)
                        r = ref.anchor_to_input(an, col[ofs + 2:ofs + 6])
                        if ref.overlaps_image(r, ref.IMG_W, ref.IMG_H):
                            out.append(((i, a, y, x), l0, r))
    return out


@pytest.mark.parametrize("pattern", ref.scan_patterns_for("n12"))
def test_scan_order_on_twelve_anchors(pattern):
    c = ref.scan_case("n12", pattern)
    w = c["want"]
    lit = _literal_scan(c)
    assert w["count"] == len(lit) and w["total"] == 12
    assert w["idx"].tolist() == [list(m[0]) for m in lit]
    for i, (_, p, r) in enumerate(lit):
        assert abs(float(w["p"][i]) - p) <= w["p_tol"][i]
        assert np.all(np.abs(w["rect"][i] - np.array(r)) <= w["rect_tol"][i])
    if pattern == "all":       # layer outermost, then (1 x 1 maps) the aspect
        assert w["idx"].tolist() == [[l, a, 1, 1] for l in range(1, 5) for a in range(1, 4)]


# ------------------------------------------------------------------------------------------------ criteria against torch
def test_rpn_loss_ref_against_torch():
    import torch
    Fn = torch.nn.functional
    seen_z = set()
    for E, npos in ref.LOSS_CASES:
        c = ref.loss_case(E, npos)
        w = c["want"]
        for e in range(E):
            l, a, y, x = (int(v) - 1 for v in c["ex_idx"][e])
            v = torch.tensor(c["maps"][l][a * 6:a * 6 + 6, y, x].astype(np.float64), requires_grad=True)
            target = torch.tensor([0 if e < npos else 1])
            loss = Fn.nll_loss(Fn.log_softmax(v[:2], 0)[None], target, reduction="sum")
            assert abs(w["ex_loss"][e, 0] - loss.item()) <= max(w["ex_loss_tol"][e, 0], ref.ulp32(loss.item()))
            if e < npos:
                tgt = torch.tensor(np.array(ref.input_to_anchor(c["ex_anchor"][e], c["ex_roi"][e]), np.float64))
                reg = Fn.smooth_l1_loss(v[2:], tgt, beta=1.0, reduction="sum") * 10
                # torch takes the difference in float64, the criterion in fp32: half an fp32 ulp of the operands per element,
                # through a derivative of at most 1, plus the rounding of the sum
                slack = 10 * (sum(0.5 * ref.ulp32(max(abs(v[2 + k].item()), abs(tgt[k].item()))) for k in range(4))
                              + ref.ulp32(reg.item() / 10))
                assert abs(w["ex_loss"][e, 1] - reg.item()) <= slack
                loss = loss + reg
                seen_z.update(float(np.float32(np.float32(v[2 + k].item()) - np.float32(tgt[k].item()))) for k in range(4))
                assert w["cctarget"][e] == c["ex_class"][e]
            else:
                assert w["ex_loss"][e, 1] == 0 and w["cctarget"][e] == ref.BGCLASS and not w["crtarget"][e].any()
            loss.backward()
            mine = [ad for ad in w["addends"] if (ad[0], ad[1]) in
                    {(l, (a * 6 + k) * c["maps"][l][0].size + y * c["maps"][l].shape[2] + x) for k in range(6)}]
            assert len(mine) == (6 if e < npos else 2)
            g = v.grad.numpy()
            for k, ad in enumerate(mine):
                # (the SmoothL1 gradient at |z| == 1: torch's float64 branch is the fp32 one, the edge values being exact)
                assert abs(ad[2] - g[k]) <= 4e-6 * max(1.0, abs(g[k])), (e, k, ad, g[k])
    # the switch of SmoothL1: all of Z_EDGES occur as exact differences among the positives
    assert set(ref.Z_EDGES) <= seen_z


def test_rpn_loss_ref_edge_values_by_hand():
    """|z| == 1 takes the linear branch (|z| - 0.5 = 0.5, gradient +-1), the fp32 below 1 the quadratic one"""
    terms, grads = ref.smooth_l1_terms([1.0, -1.0, ref.ONE_M, -ref.ONE_M, 0.0, 3.0, -3.0])
    assert terms == [0.5, 0.5, 0.5 * ref.ONE_M ** 2, 0.5 * ref.ONE_M ** 2, 0.0, 2.5, 2.5]
    assert grads == [1.0, -1.0, ref.ONE_M, -ref.ONE_M, 0.0, 1.0, -1.0]
    assert ref.f32(ref.ONE_M) == ref.ONE_M and ref.ONE_M < 1.0


def test_expected_maps_sums():
    d0 = [np.full((18, 1, 1), 1.0, np.float32) for _ in range(4)]
    add = [(2, 5, 2.0 ** -24, 0.0), (2, 5, 2.0 ** -24, 0.0), (2, 5, -1.0, 0.0), (0, 0, 0.5, 1e-9)]
    seq = ref.expected_maps(d0, add, "f32seq")
    assert seq[2][5, 0, 0] == 0.0 and seq[0][0, 0, 0] == 1.5       # 1 + 2^-24 rounds back to 1, twice
    want, bound = ref.expected_maps(d0, add, "f64")
    assert want[2][5, 0, 0] == 2.0 ** -23 and bound[2][5, 0, 0] == 4 * 2.0 ** -24 * (2 + 2.0 ** -23)
    assert bound[0][0, 0, 0] == 2 * 2.0 ** -24 * 1.5 + 1e-9 and bound[1].max() == 0


def test_cnet_losses_ref_against_torch():
    import torch
    Fn = torch.nn.functional
    for R in ref.CNET_R:
        for npos in ref.cnet_npos(R):
            for ncls in ref.CNET_NCLS:
                c = ref.cnet_losses_case(R, npos, ncls)
                w = c["want"]
                cr = torch.tensor(w["crout"].astype(np.float64), requires_grad=True)
                cc = torch.tensor(c["ccout"].astype(np.float64), requires_grad=True)
                reg = Fn.smooth_l1_loss(cr, torch.tensor(c["crtarget"].astype(np.float64)), beta=1.0, reduction="sum")
                cls = Fn.nll_loss(cc, torch.tensor(c["cctarget"].astype(np.int64) - 1))
                (reg * 10 + cls).backward()
                assert abs(w["cls_mean"] - cls.item()) <= 1e-13 * max(1.0, abs(cls.item()))
                assert np.array_equal(w["ccdelta"], cc.grad.numpy().astype(np.float32))
                # torch's difference is float64, the criterion's fp32
                assert abs(w["reg_sum"] - reg.item()) <= 4 * R * 1e-6
                g = cr.grad.numpy()
                z = w["crout"].astype(np.float64) - c["crtarget"]
                smooth = np.abs(np.abs(z) - 1.0) > 1e-6
                assert np.all(np.abs(w["crdelta"] - g)[smooth] <= 2e-5)
                assert np.all(np.abs(w["crdelta"]) <= 10.0)
                assert np.array_equal(w["crout"][:npos], c["crout"][:npos]) and not w["crout"][npos:].any()


def test_decode_ref_first_maximum():
    x = np.array([[-1, -0.5, -0.5, -2], [-3, -3, -3, -3], [-2, -1, -1, -0.25]], np.float32)
    cls, conf = ref.decode_ref(x)
    assert cls.tolist() == [2, 1, 4] and conf.tolist() == [-0.5, -3.0, -0.25]
    import torch
    for R in ref.DECODE_R:
        for ncls in ref.DECODE_NCLS:
            for kind in ref.DECODE_KINDS:
                x = ref.decode_case(R, ncls, kind)
                cls, conf = ref.decode_ref(x)
                assert np.array_equal(conf, x.max(1)) and np.array_equal(cls, np.argmax(x, 1) + 1)


# ------------------------------------------------------------------------------------------------ input conditions of the GPU tests
@pytest.mark.parametrize("name", sorted(ref.SCAN_SIZES))
def test_scan_problems_meet_their_input_conditions(name):
    sizes = ref.SCAN_SIZES[name]
    total = ref.scan_total(name)
    assert total == {"n12": 12, "n1023": 1023, "n1026": 1026, "n2490": 2490, "n1287": 1287}[name]
    if name != "n12":
        assert all(h != w for h, w in sizes) and len(set(sizes)) == 4          # non-square, every layer another size
    pats = ref.scan_patterns_for(name)
    assert set(pats) >= {"none", "all", "first", "last", "alternate", "random", "soft"}
    assert ("a63_a64" in pats) == (total > 65) and ("a1023_a1024" in pats) == (total > 1025) and ("wave1" in pats) == (total > 128)
    kinds_seen = set()
    for p in pats:
        c = ref.scan_case(name, p)
        w = c["want"]
        assert w["total"] == total
        assert w["thr_margin"].min() > ref.MARGIN, "an exp(c1) within 1e-6 of the threshold"
        assert w["ovl_margin"].min() > ref.MARGIN, "a rect within 1e-6 of the image size of a border"
        assert np.all(np.diff(c["aw"], axis=2) > 0) and np.all(np.diff(c["ah"], axis=2) > 0) and c["aw"].dtype == np.float32
        # the logits: +-30 exactly, and the flags are what the threshold test sees
        v0 = np.concatenate([m.reshape(3, 6, -1)[:, 0].T.ravel() for m in c["maps"]])
        if p == "soft":        # logits of order 1: p is of the order of its own bound's scale
            assert np.abs(v0).max() <= 1 and w["count"] > 0
            assert np.all(w["p"] < -0.005) and np.all(w["p"] > -0.05) and w["p_tol"].max() <= 2 * ref.ulp32(7.0)
        else:
            assert np.array_equal(np.abs(v0), np.full(total, 30.0, np.float32)) and np.array_equal(v0 > 0, c["flags"])
        b = c["border"]
        if p in ("alternate", "random", "soft"):
            on = c["flags"]
            if total > 100:
                for kind in range(8):
                    sel = b == kind
                    assert sel.sum() >= 3
                    assert np.all(w["match"][sel] == bool(kind % 2)), "just outside must miss, just inside must match"
                    side = kind // 2
                    size = (ref.IMG_W, ref.IMG_W, ref.IMG_H, ref.IMG_H)[side]
                    assert np.all(np.abs(w["ovl_margin"][sel, side] * size - ref.BORDER) < 1e-3)
                kinds_seen.update(range(8))
            assert 0 < w["count"] < on.sum()
        else:
            assert np.array_equal(w["match"], c["flags"]), "the pattern must reach the compaction as it is"
            assert w["count"] == {"none": 0, "all": total, "first": 1, "last": 1, "a63_a64": 2, "a1023_a1024": 2, "wave1": 64}[p]
        caps = ref.scan_caps(w["count"], total)
        assert caps[0] == 0 and caps[2] == w["count"] and caps[3] > total and caps[1] == max(w["count"] - 1, 0)
    if total > 100:
        assert kinds_seen == set(range(8))
    if name == "n1287":       # the last entries of both tables are read
        c = ref.scan_case(name, "all")
        assert c["want"]["idx"][:, 2].max() == 200 and c["want"]["idx"][:, 3].max() == 200


def test_loss_problems_meet_their_input_conditions():
    assert [E for E, _ in ref.LOSS_CASES[:5]] == [1, 63, 64, 65, 300]
    assert any(npos == 0 for _, npos in ref.LOSS_CASES) and any(npos == E for E, npos in ref.LOSS_CASES[5:])
    sizes = ref.LOSS_SIZES
    corners = {(l + 1, a + 1, y, x) for l in range(4) for a in range(3) for y, x in ((1, 1), sizes[l])}
    for E, npos in ref.LOSS_CASES:
        c = ref.loss_case(E, npos)
        keys = [tuple(int(v) for v in k) for k in c["ex_idx"]]
        assert len(set(keys)) == E, "distinct anchors"
        if E >= 24:
            assert corners <= set(keys)
        for d0 in c["deltas0"]:
            assert np.all(d0 != 0)
        gaps = set()
        for e, (l, a, y, x) in enumerate(keys):
            m = c["maps"][l - 1]
            gaps.add(float(m[(a - 1) * 6 + 1, y - 1, x - 1]) - float(m[(a - 1) * 6, y - 1, x - 1]))
        if E >= 63:
            assert 0.0 in gaps and any(abs(abs(g) - 100) < 1e-3 for g in gaps) and any(abs(abs(g) - 1e4) < 1 for g in gaps)
            assert any(g > 50 for g in gaps) and any(g < -50 for g in gaps)
    for k in ref.DUP_CASES:
        c = ref.loss_case(ref.DUP_E, ref.DUP_NPOS, k)
        keys = [tuple(int(v) for v in key) for key in c["ex_idx"]]
        counts = sorted((keys.count(key) for key in set(keys)), reverse=True)
        assert counts[:ref.DUP_ANCHORS + 1] == [k + 2] + [k] * (ref.DUP_ANCHORS - 1) + [1], counts
        assert sorted(keys[:c["npos"]].count(key) for key in set(keys[:c["npos"]]))[-ref.DUP_ANCHORS:] == [k] * ref.DUP_ANCHORS
        w = c["want"]
        # every addend is exact, regression addends at a repeated address differ from one another, and the fp32 sum in example
        # order is not the sum in the opposite order everywhere: the order is observable
        per = {}
        for l, off, a, tol in w["addends"]:
            per.setdefault((l, off), []).append((a, tol))
        rep = {key: v for key, v in per.items() if len(v) > 1}
        assert len(rep) == 6 * ref.DUP_ANCHORS
        assert sum(len({a for a, _ in v}) > 1 for v in rep.values()) >= 2 * ref.DUP_ANCHORS
        assert not w["ex_loss_tol"].any()
        fwd = ref.expected_maps(c["deltas0"], w["addends"], "f32seq")
        bwd = ref.expected_maps(c["deltas0"], w["addends"][::-1], "f32seq")
        assert any(not np.array_equal(a, b) for a, b in zip(fwd, bwd))


def test_accumulate_problems_span_twelve_decades():
    assert ref.ACC_E == (1, 63, 64, 65, 300, 0)
    for E in ref.ACC_E:
        ex, acc0 = ref.accumulate_case(E)
        assert ex.shape == (E, 2) and np.all(acc0 != 0)
        if E >= 63:
            mag = np.abs(ex)
            assert mag.max() / mag.min() >= 1e12 * (1 - 1e-9)


def test_cnet_and_decode_problems_meet_their_input_conditions():
    for R in ref.CNET_R:
        assert ref.cnet_npos(R)[0] == 0 and ref.cnet_npos(R)[-1] == R and (R == 1 or 0 < ref.cnet_npos(R)[1] < R)
        for npos in ref.cnet_npos(R):
            for ncls in ref.CNET_NCLS:
                c = ref.cnet_losses_case(R, npos, ncls)
                z = (c["want"]["crout"] - c["crtarget"]).astype(np.float32).ravel()
                n = min(R * 4, 2 * len(ref.CNET_Z))
                assert z[:n].tolist() == [ref.f32(ref.CNET_Z[i % len(ref.CNET_Z)]) for i in range(n)]
                t = c["cctarget"]
                assert t.min() >= 1 and t.max() <= ncls and ncls in t and (R == 1 or 1 in t)
                assert np.all(c["loss0"] != 0)
    for ncls in ref.DECODE_NCLS[1:]:
        x = ref.decode_case(300, ncls, "quantised")
        ties = sum(int((row == row.max()).sum() > 1) for row in x)
        assert ties > 30, "exact ties must be frequent"
        x = ref.decode_case(300, ncls, "last_column")
        assert np.all(ref.decode_ref(x)[0] == ncls)
    assert np.all(ref.decode_ref(ref.decode_case(65, 17, "all_equal"))[0] == 1)
