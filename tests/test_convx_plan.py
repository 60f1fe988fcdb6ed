"""The tables of tests/test_gpu_convx_plans.py reach every launch plan of the split-operand convolutions they exist for
(tests/convx_plan.py restates the host-side shape rules of csrc/convx.hip and csrc/wgradx.hip; no GPU needed).  A later
edit of the tables cannot drop a branch without this failing.  Also: the share of the operands' representation in the
error bound of the GPU file, checked against both splits emulated in numpy."""
import numpy as np
import pytest

import conv_plan as CP
import convx_plan as XP
import width_plan as WP


def test_restatement_at_known_values():
    """values read off the C++ (convx.hip conv_x3 / x3_choose_tile / conv_x3_bm, wgradx.hip wgradx_plan)"""
    assert [XP.cx_pp(k) for k in (3, 5, 7)] == [204, 240, 308]

    def x3(shape):
        p = XP.x3_plan(shape)
        return (p["TH"], p["TW"]), p["bm"], p["splitK"]
    # two splits of 5 + 4 chunks
    p = XP.x3_plan((144, 12, 16, 128, 3, 1))
    assert x3((144, 12, 16, 128, 3, 1)) == ((12, 8), 128, 2) and (p["chunksPerSplit"], p["lastSplitChunks"]) == (5, 4)
    assert x3((1024, 8, 8, 128, 3, 1)) == ((8, 8), 128, 16)        # the 3x3 cap
    assert x3((384, 9, 12, 128, 7, 0)) == ((3, 6), 128, 24)        # the 5x5 / 7x7 cap
    p = XP.x3_plan((16, 128, 256, 128, 3, 1))                      # the fill rule: 512 blocks of 64 filters
    assert (p["why"], p["blocks"], p["splitK"]) == ("fill_rule", 512, 1) and x3((16, 128, 256, 128, 3, 1))[:2] == ((8, 16), 64)
    assert x3((16, 3, 3, 64, 3, 0)) == ((1, 1), 64, 1)             # one output pixel
    p = XP.x3_plan((128, 13, 15, 128, 3, 1))                       # split K with the scalar fold
    assert x3((128, 13, 15, 128, 3, 1)) == ((13, 8), 128, 2) and p["vec"] == 1 and not p["wide"]
    # vgg_small's 113x200 layers, the ones conv_x3_bm's rule was made for: 190 tiles of 6x20 (widths are multiples of 4 since
    # the wide epilogue), 380 -> 760 blocks; b2c2 at 225x400 keeps 128-filter blocks
    p = XP.x3_plan((128, 113, 200, 256, 3, 1))
    assert (p["TH"], p["TW"], p["why"], p["blocks"], p["splitK"]) == (6, 20, "fill_rule", 760, 1)
    assert XP.x3_plan((128, 225, 400, 128, 3, 1))["bm"] == 128
    # the 5x5 anchor net at the benchmarked size: 24 blocks, 12 splits of two chunks; 144 channels on a small map: one chunk each
    p = XP.x3_plan((384, 29, 50, 256, 5, 0))
    assert (p["blocks"], p["chunksPerSplit"], p["splitK"]) == (24, 2, 12)
    p = XP.x3_plan((144, 9, 12, 128, 5, 0))
    assert (p["chunksPerSplit"], p["splitK"]) == (1, 9)
    # the 7x7 anchor net at the benchmarked size: 8x16-pixel tiles, 24 splits
    p = XP.x3_plan((384, 29, 50, 256, 7, 0))
    assert (p["TH"], p["TW"], p["splitK"]) == (8, 16, 24)

    def wg(shape):
        p = XP.wgradx_plan(shape)
        return p["nSplit"], p["nT"], (p["adv_x"], p["adv_y"])
    assert wg((512, 12, 40, 512, 3, 1)) == (4, [3, 2, 2, 2], (1, 1))
    n, nT, adv = wg((256, 16, 40, 512, 3, 1))
    assert (n, adv[0]) == (8, 2) and set(nT) == {1, 2}
    n, nT, adv = wg((128, 60, 80, 128, 3, 1))
    assert (n, adv[0]) == (64, 4)
    # b2c2 of vgg_small: 64 splits over 57 x 25 tiles
    assert wg((128, 225, 400, 128, 3, 1))[0] == 64
    assert XP.wgradx_loader(XP.wgradx_plan((64, 21, 34, 64, 3, 1))) == 2
    assert XP.wgradx_loader(XP.wgradx_plan((64, 21, 34, 64, 3, 1)), slack=False) == 0
    assert XP.wgradx_loader(XP.wgradx_plan((64, 21, 36, 64, 3, 1)), slack=False) == 1
    assert XP.wgradx_loader(XP.wgradx_plan((64, 21, 36, 64, 3, 1)), aligned=False) == 2
    assert XP.wgradx_loader(XP.wgradx_plan((64, 21, 36, 64, 3, 0))) == 0


def test_case_names_are_unique_and_cases_are_small():
    for table in (XP.X3_CASES, XP.WG_CASES):
        names = [c["name"] for c in table]
        assert len(names) == len(set(names))
    for c in XP.X3_CASES + XP.WG_CASES:
        C, H, W, O, k, pad = c["shape"]
        assert (H + 2 * pad - k + 1) * (W + 2 * pad - k + 1) <= 35000 and O * C * k * k * 4 <= 10e6, c["name"]
    for n in XP.X3_NO_BIAS + XP.X3_MISALIGNED + [n for n, _ in XP.X3_ACT] + [n for n, _, _ in XP.X3_POST]:
        XP.find_x3(n)
    for n, m in XP.X3_ACT:
        assert XP.find_x3(n)["shape"][4] == 3 and m in XP.ACT_MODES     # (api.cpp: only 3x3 launches take an activation)
    for n, m in XP.WG_ACT:
        assert XP.find_wg(n) and m in XP.ACT_MODES


def test_cases_reach_what_they_are_listed_for():
    for c in XP.X3_CASES:
        labels = set()
        for r in XP.x3_runs():
            if r["name"] == c["name"] and r.get("out_aligned", True) and r["role"] != "post" and not r.get("act"):
                labels |= XP.x3_labels_of_run(r)
        assert c["want"] <= labels, (c["name"], sorted(c["want"] - labels))
    for c in XP.WG_CASES:
        labels = XP.wg_labels_of_run(dict(shape=c["shape"], place=c["place"], act=None))
        assert c["want"] <= labels, (c["name"], sorted(c["want"] - labels))


def _reached(x3_runs, wg_runs):
    """label -> the shapes that reach it"""
    out = {}
    for r in x3_runs:
        for l in XP.x3_labels_of_run(r):
            out.setdefault(l, set()).add(r["shape"])
    for r in wg_runs:
        for l in XP.wg_labels_of_run(r):
            out.setdefault(l, set()).add(r["shape"])
    return out


def _short(x3_runs, wg_runs):
    """required labels reached by fewer shapes than they should be"""
    got = _reached(x3_runs, wg_runs)
    return sorted(l for l in XP.REQUIRED if len(got.get(l, ())) < XP.FEWER_THAN_TWO.get(l, 2))


def test_every_required_label_is_reached_by_two_shapes():
    assert _short(XP.x3_runs(), XP.wg_runs()) == []
    assert set(XP.FEWER_THAN_TWO) <= XP.REQUIRED


def test_removing_a_case_that_a_label_depends_on_is_noticed():
    x3, wg = XP.x3_runs(), XP.wg_runs()
    got = _reached(x3, wg)
    tight = [l for l in sorted(XP.REQUIRED) if len(got[l]) == XP.FEWER_THAN_TWO.get(l, 2)]
    assert {"bm64_fill_rule", "splitk_cap16", "splitk_cap24", "splits_recomputed", "wg_one_tile", "wg_nt4plus",
            "wg_vec0_no_slack"} <= set(tight)
    for label in tight:     # every shape such a label rests on: without it the label is reported
        for shape in got[label]:
            short = _short([r for r in x3 if r["shape"] != shape], [r for r in wg if r["shape"] != shape])
            assert label in short, (label, shape)
    # a variant list emptied
    assert "narrow_misaligned" in _short([r for r in x3 if r.get("out_aligned", True) and r.get("post_aligned", True)], wg)
    assert "post_fold_vec2" in _short([r for r in x3 if r["role"] != "post"], wg)
    assert "wg_act_slope" in _short(x3, [r for r in wg if r["act"] is None])


def test_the_mirrored_input_gradient_is_the_same_launch():
    for c in XP.X3_CASES:
        C, H, W, O, k, pad = c["shape"]
        mC, mH, mW, mO, mk, mpad = CP.mirror(c["shape"])
        # api.cpp frcnn_conv2d_backward_input: conv_x3 with K channels = the op's filters, M = its channels, pad' = k - 1 - pad
        assert WP.conv_x3_eligible(mO, mC, mk)
        Ho, Wo = mH + 2 * mpad - mk + 1, mW + 2 * mpad - mk + 1
        assert (mO, Ho, Wo, mC, mk, mk - 1 - mpad) == c["shape"], c["name"]
        assert CP.takes_split_form("forward", c["shape"]) and CP.takes_split_form("input_gradient", CP.mirror(c["shape"]))
    for c in XP.WG_CASES:
        assert CP.takes_split_form("weight_gradient", c["shape"])


def test_chosen_tiles_fit_the_block():
    """every chosen tile has at most 128 pixels and a patch plane the block can stage; a 3x3 tile is cut by the patch plane
    only on tall maps narrower than 8 pixels"""
    for k in (3, 5, 7):
        for Ho in range(1, 65):
            for Wo in range(1, 161):
                th, tw, cut = XP.x3_choose_tile(Ho, Wo, k)
                assert th * tw <= XP.CX_NTMAX and (th + k - 1) * (tw + k - 1) <= XP.cx_pp(k)
                assert k != 3 or not cut or (Wo < 8 and Ho >= 48)
    assert XP.x3_choose_tile(48, 3, 3) == (38, 3, True)


def test_tile_walk_of_the_weight_gradient():
    """wgradx_plan() asserts the division-free walk against t = split + i nSplit; the wrap is a step with tx + adv_x >= tilesX"""
    for O in (64, 128, 512):
        for H in range(1, 40, 3):
            for W in range(1, 100, 7):
                p = XP.wgradx_plan((64, H, W, O, 3, 1))
                assert sum(p["nT"]) == p["npix"] and min(p["nT"]) >= 1 and max(p["nT"]) - min(p["nT"]) <= 1
                assert p["wraps"] <= (p["adv_x"] > 0)
    kinds = {(XP.wgradx_plan(c["shape"])["adv_x"] > 0, XP.wgradx_plan(c["shape"])["wraps"]) for c in XP.WG_CASES}
    assert (True, True) in kinds and (False, False) in kinds


# ---- the representation share of the bound ---------------------------------------------------------------------------------
def _ops(shape):
    C, H, W, O, k, pad = shape
    fwd = lambda x, w: CP.ref_forward(x, w, None, pad)                    # noqa: E731
    wgr = lambda x, g: CP.ref_weight_gradient(x, g, k, pad)[0]            # noqa: E731
    return fwd, wgr


_share = XP.representation_share


CROP = 64   # filters (and, in the weight gradient, channels) whose outputs are checked: the full tensors' magnitudes scale the planes


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16x6", "f16x3"])
def test_representation_share_of_the_bound(f16):
    """both splits emulated in numpy, the kept products summed in fp64: the distance to the fp64 reference stays inside
    representation_bound for every case (forward operands; the input gradient splits the same two kinds of tensor).  Of a
    large case the outputs of the first CROP filters (x CROP channels) are taken: an output depends on its own rows of the
    operands and, with two planes, on the whole tensors' largest magnitudes, which are passed along."""
    worst = 0.0
    for c in XP.X3_CASES:
        C, H, W, O, k, pad = c["shape"]
        rng = np.random.RandomState(C + H + W + O + k)
        x = rng.randn(C, H, W).astype(np.float32)
        w = (rng.randn(O, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
        worst = max(worst, _share(_ops(c["shape"])[0], x, w[:CROP], f16, c["name"], np.abs(x).max(), np.abs(w).max()))
    for c in XP.WG_CASES:
        C, H, W, O, k, pad = c["shape"]
        rng = np.random.RandomState(C + H + W + O)
        x = rng.randn(C, H, W).astype(np.float32)
        g = (rng.randn(O, H + 2 * pad - 2, W + 2 * pad - 2) / np.sqrt(H * W)).astype(np.float32)
        worst = max(worst, _share(_ops(c["shape"])[1], x[:CROP], g[:CROP], f16, c["name"], np.abs(x).max(), np.abs(g).max()))
    print("largest distance / representation share: %.3f" % worst)
    assert worst > 0.01   # (the share is no empty claim: the emulated splits do use a visible part of it)


def test_representation_share_with_a_fused_activation_and_wide_range():
    """the fp16 form under a dropout scale leaves one binade of headroom (top = 13) and scales by the RAW tensor's magnitude;
    magnitudes spread over many binades reach the subnormal floor 2^-38 amax"""
    shape = XP.find_x3("ragged_bm128")["shape"]
    C, H, W, O, k, pad = shape
    rng = np.random.RandomState(7)
    x = rng.randn(C, H, W).astype(np.float32)
    w = (rng.randn(O, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    scale = (rng.rand(C) > 0.4).astype(np.float32)
    act = CP.activate(x, 0.25, scale)
    _share(_ops(shape)[0], act, w, 1, "act both", amax_a=np.abs(x).max(), top_a=13)
    xw = (rng.randn(C, H, W) * np.exp(3 * rng.randn(C, H, W))).astype(np.float32)
    ww = (w * np.exp(2 * rng.randn(*w.shape))).astype(np.float32)
    for f16 in (0, 1):
        _share(_ops(shape)[0], xw, ww, f16, "wide range")


def test_plane_emulation():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -3.14159274, 1e-30, 0.0, 65504.0 * 4], np.float32)
    assert np.array_equal(XP.bf16_round(x[:3]), np.array([1.0, 1.0, 1.0 + 2.0 ** -7], np.float32))   # ties to even
    h, m, l = XP.planes_bf16(x)
    assert np.all(np.abs(h + m + l - x.astype(np.float64)) <= 2.0 ** -26 * np.abs(x))
    (h, l), e = XP.planes_f16(x)
    assert e == 14 - 17 and np.all(np.isfinite(h))
    assert np.all(np.abs((h + l) * 2.0 ** -e - x.astype(np.float64)) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -38 * np.abs(x).max())
    assert XP.f16_exponent(0.0) == 0 and XP.f16_exponent(1.0) == 14 and XP.f16_exponent(1.99, 13) == 13 and XP.f16_exponent(2.0) == 13
