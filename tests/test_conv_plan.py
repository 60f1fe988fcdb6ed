"""The tables of tests/test_gpu_conv_plans.py reach every launch plan of the fp32 matrix-core convolutions they exist
for (tests/conv_plan.py restates csrc/conv.hip's host-side shape rules; no GPU needed).  A later edit of the tables
cannot drop a branch without this failing.  Also: which cases of tests/test_gpu_conv.py still reach conv.hip with the
default options, and the fp64 references of the GPU file against the CPU oracle."""
import ast
import os

import numpy as np
import pytest

import conv_plan as CP

ROLES = ("forward", "input_gradient")


def _igemm_plan(role, c):
    return CP.forward_plan(c["shape"]) if role == "forward" else CP.input_gradient_plan(CP.mirror(c["shape"]))


def test_restatement_at_known_values():
    assert [CP.conv_cc(k) for k in (1, 3, 5, 7)] == [32, 8, 2, 2]
    assert [CP.conv_mpad(M) for M in (1, 64, 65, 128, 129, 512)] == [64, 64, 128, 128, 256, 512]
    # b2c2 of vgg_small (128 -> 128 on 225x400): "one wave of 1440 blocks, no split" (tests/test_gpu_conv.py FULL_LAYERS)
    p = CP.igemm_plan(128, 225, 400, 128, 3, 1)
    assert (p["blocks"], p["splitK"], p["BM"]) == (1440, 1, 64)
    # the 7x7 anchor net (384 -> 256 on 29x50, valid): 24 splits
    assert CP.igemm_plan(384, 29, 50, 256, 7, 0)["splitK"] == 24
    # the 1x1 head with M = 18: 64-row tiles; a 1x1 launch with more filters: 128-row tiles
    assert CP.igemm_plan(256, 55, 98, 18, 1, 0)["BM"] == 64 and CP.igemm_plan(256, 55, 98, 65, 1, 0)["BM"] == 128
    # the first layer's weight gradient (3 -> 64 on 450x800): 13 x 113 tiles of 4x64, capped at 512 slabs, the tall fold
    p = CP.wgrad_plan(3, 450, 800, 64, 3, 1)
    assert (p["kernel"], p["tilesX"] * p["tilesY"], p["nSplit"], p["fold"]) == ("first", 13 * 113, 512, "tall")
    # ... and the shape of the stale-flag report: 10 slabs with the first-layer kernel, 38 with the generic one
    assert CP.wgrad_plan(3, 37, 53, 64, 3, 1)["nSplit"] == 10 and CP.wgrad_plan(3, 37, 53, 64, 3, 1, act=True)["nSplit"] == 38
    assert CP.wgrad_workspace_floats((3, 37, 53, 64, 3, 1)) == 38 * 9 * 64 * 3


def test_case_names_are_unique():
    names = [c["name"] for c in CP.IGEMM_CASES + CP.SPLITK_CASES + CP.WGRAD_CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("role", ROLES)
def test_igemm_cases_reach_what_they_are_listed_for(role):
    reached = set()
    for c in CP.IGEMM_CASES + CP.SPLITK_CASES:
        labels = CP.igemm_labels(_igemm_plan(role, c))
        assert c["want"] <= labels, (role, c["name"], sorted(c["want"] - labels))
        reached |= labels
    assert CP.IGEMM_REQUIRED <= reached, sorted(CP.IGEMM_REQUIRED - reached)


def test_the_mirrored_input_gradient_takes_the_forward_plan():
    for c in CP.IGEMM_CASES + CP.SPLITK_CASES:
        C, H, W, O, k, pad = c["shape"]
        m = CP.mirror(c["shape"])
        assert CP.input_gradient_plan(m) == CP.forward_plan(c["shape"]), c["name"]
        assert m[5] >= 0 and (m[1] + 2 * m[5] - k + 1, m[2] + 2 * m[5] - k + 1) == (H, W)   # its gradient map is the forward's input map


def test_filter_and_channel_counts_of_the_issue():
    by_k = {k: [c["shape"] for c in CP.IGEMM_CASES if c["shape"][4] == k] for k in (1, 3, 5, 7)}
    for k in (1, 3, 5, 7):
        assert {1, 18, 63, 64, 65, 128, 129} <= {s[3] for s in by_k[k]}, k
    assert {1, 3, 4, 5, 9} <= {s[0] for s in by_k[3]}
    assert {31, 33, 130} <= {s[0] for s in by_k[1]}
    assert {5, 13, 17} <= {s[0] for s in by_k[5]} and {5, 13, 17} <= {s[0] for s in by_k[7]}
    assert {CP.forward_plan(s)["BM"] for s in by_k[1]} == {64, 128}
    for k in (3, 5, 7):
        assert {CP.forward_plan(s)["BM"] for s in by_k[k]} == {64}
    # Cin <= 4 is the first-layer instantiation, 5 is not
    assert [CP.forward_plan(CP.find("c%d_k3" % c)["shape"])["first"] for c in (1, 3, 4, 5, 9)] == [True, True, True, False, False]
    # 5x5 and 7x7: one case in each patch-plane class
    for k in (5, 7):
        assert {CP.forward_plan(s)["NIT"] for s in by_k[k]} == {1, 2, 4}, k
    assert CP.forward_plan(CP.find("row_k7")["shape"])["NIT"] == 4


def test_split_k_cases():
    for c in CP.SPLITK_CASES:
        p = CP.forward_plan(c["shape"])
        got = (p["splitK"], p["chunksPerSplit"], p["lastSplitChunks"], p["lastChunkChannels"])
        assert got == CP.SPLITK_WANT[c["name"]], (c["name"], got)
        assert p["blocks"] == p["mTiles"] and p["tilesX"] == p["tilesY"] == 1   # one tile: split K at small cost
        assert p["fold"] == "splitk_reduce"
    assert set(CP.SPLITK_WANT) == {c["name"] for c in CP.SPLITK_CASES}
    # what the seven small shapes of tests/test_gpu_conv.py (the ones that reach conv.hip by default) do: forward only 130 -> 130
    # splits K (5 slabs of 4,4,4,4,1 chunks); the input gradient (test_conv_backward_input runs CASES[1:]) also at the 5x5 and
    # 7x7 heads.  No 1x1 split, no split with a bias-less forward, none at the cap.
    small = [s for s in CP.GPU_CONV_CASES if not CP.takes_split_form("forward", s)]
    assert [CP.forward_plan(s)["splitK"] for s in small] == [1, 1, 1, 1, 1, 1, 5]
    assert [CP.input_gradient_plan(s)["splitK"] for s in small[1:]] == [1, 1, 1, 3, 4, 5]
    assert all(CP.forward_plan(s)["splitK"] == 1 for s in small if s[4] == 1)


def test_activation_cases():
    for k, names in CP.ACT_SHAPES.items():
        split, one = (CP.find(n)["shape"] for n in names)
        assert split[4] == one[4] == k
        ps, po = CP.forward_plan(split, act=True), CP.forward_plan(one, act=True)
        assert ps["splitK"] > 1 and po["splitK"] == 1 and ps["loader"] == po["loader"] == "act"
        for s in (split, one):   # the entry point sends these to conv.hip whatever split_bf16 says
            assert not CP.takes_split_form("forward", s, act=True)
    for name, mode in CP.ACT_EXTRA:
        assert mode in CP.ACT_MODES and CP.find(name)
    assert CP.forward_plan(CP.find("c3_k3")["shape"], act=True)["first"]
    assert CP.forward_plan(CP.find("split_k1_bm128")["shape"], act=True)["BM"] == 128
    for name in CP.ACT_SCALE_TWO:
        assert CP.find(name)


def test_wgrad_cases_reach_what_they_are_listed_for():
    reached = set()
    for c in CP.WGRAD_CASES:
        labels = CP.wgrad_labels(CP.weight_gradient_plan(c["shape"]))
        assert c["want"] <= labels, (c["name"], sorted(c["want"] - labels))
        reached |= labels
    assert CP.WGRAD_REQUIRED <= reached, sorted(CP.WGRAD_REQUIRED - reached)
    first = [c["shape"] for c in CP.WGRAD_CASES if CP.weight_gradient_plan(c["shape"])["kernel"] == "first"]
    assert {s[0] for s in first} == {1, 2, 3} and {1, 17, 64} <= {s[3] for s in first}
    slabs = sorted(CP.weight_gradient_plan(s)["nSplit"] for s in first)
    assert slabs[0] == 1 and 127 in slabs and 128 in slabs and slabs[-1] == 512
    assert CP.weight_gradient_plan(CP.find("first_cap")["shape"])["tilesPerBlock"] == 2
    generic = [CP.weight_gradient_plan(c["shape"]) for c in CP.WGRAD_CASES if "generic" in c["want"]]
    for k in (1, 3, 5, 7):
        ps = [p for p in generic if p["k"] == k]
        assert {p["nSplit"] == 1 for p in ps} == {True, False}, k
        assert {1, 63, 65, 130} & {p["O"] for p in ps} and {1, 63, 65, 130} & {p["Cin"] for p in ps}
    assert {1, 63, 65, 130} <= {p["O"] for p in generic} and {1, 63, 65, 130} <= {p["Cin"] for p in generic}
    # the three neighbours of the first-layer predicate: one term fails each
    assert CP.weight_gradient_plan(CP.find("near_first_wo1")["shape"])["Wo"] == 1
    assert CP.find("near_first_o65")["shape"][3] == 65 and CP.find("near_first_c4")["shape"][0] == 4


def test_three_patch_slots_belong_to_3x3_only():
    """launch_wgrad takes the three-slot kernel when the staged patch plane exceeds 128 positions.  With tiles of at most 64
    pixels and one tap row per block (k = 1, 5, 7) the plane is TH * (TW + k - 1) <= 64 + 8 * 6 = 112: only the 3x3
    kernel, which stages TH + 2 rows, gets there."""
    for k in (1, 5, 7):
        for Ho in range(1, 40):
            for Wo in range(1, 80):
                th, tw = CP.choose_wgrad_tile(Ho, Wo, k, 1)
                assert th * (tw + k - 1) <= 128
    assert CP.weight_gradient_plan(CP.find("k3_wide_tiles")["shape"])["PM"] == 3


def test_wgrad_activation_cases():
    ks = set()
    for name in CP.WGRAD_ACT_CASES:
        s = CP.find(name)["shape"]
        p = CP.weight_gradient_plan(s, act=True)
        assert p["kernel"] == "generic", name     # the first-layer kernel has no activating loader
        assert not CP.takes_split_form("weight_gradient", s)
        ks.add(p["k"])
        assert CP.wgrad_workspace_floats(s) >= p["slab_floats"]
    assert ks == {1, 3, 5, 7}
    s = CP.find("first_c3_o64")["shape"]
    assert s == (3, 37, 53, 64, 3, 1)
    assert CP.weight_gradient_plan(s)["kernel"] == "first"
    # the generic plan of this shape needs more slabs than the first-layer plan: a workspace sized for one does not hold the other
    assert CP.weight_gradient_plan(s, act=True)["slab_floats"] > CP.weight_gradient_plan(s)["slab_floats"]
    assert {3} <= {CP.weight_gradient_plan(CP.find(n)["shape"], act=True)["PM"] for n in CP.WGRAD_ACT_CASES}


def test_order_pairs_name_cases_of_every_kernel_family():
    fams = set()
    for ra, a, acta, rb, b, actb in CP.ORDER_PAIRS:
        for role, name, act in ((ra, a, acta), (rb, b, actb)):
            s = CP.find(name)["shape"]
            assert act in (None,) + CP.ACT_MODES
            if role == "weight_gradient":
                p = CP.weight_gradient_plan(s, act is not None)
                fams.add("wgrad_" + p["kernel"] + ("_tall" if p["fold"] == "tall" else ""))
            else:
                p = CP.forward_plan(s, act is not None)   # (the mirrored input gradient has the same plan)
                fams.add("igemm_k%d%s" % (p["k"], "_splitk" if p["splitK"] > 1 else ""))
        assert (ra, a, acta) != (rb, b, actb)
    assert {"igemm_k1_splitk", "igemm_k3_splitk", "igemm_k5_splitk", "igemm_k7_splitk", "wgrad_first", "wgrad_first_tall",
            "wgrad_generic"} <= fams, sorted(fams)
    # the first-layer weight gradient with and without an activation, in both orders
    fl = [(a, acta, b, actb) for ra, a, acta, rb, b, actb in CP.ORDER_PAIRS if a == b == "first_c3_o64"]
    assert sorted(fl, key=str) == sorted([("first_c3_o64", None, "first_c3_o64", "slope"), ("first_c3_o64", "slope", "first_c3_o64", None)], key=str)


def _literal_cases(path, name="CASES"):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name:
            return [tuple(t) for t in ast.literal_eval(node.value)]
    raise AssertionError("%s not found in %s" % (name, path))


def test_which_cases_of_test_gpu_conv_still_reach_conv_hip():
    """With option split_bf16 at its default (on), the eligible shapes go to convx.hip / wgradx.hip."""
    here = os.path.dirname(os.path.abspath(__file__))
    cases = _literal_cases(os.path.join(here, "test_gpu_conv.py"))
    assert cases == CP.GPU_CONV_CASES
    split = {role: [s for s in cases if CP.takes_split_form(role, s)] for role in ("forward", "input_gradient", "weight_gradient")}
    big = [(64, 57, 100, 128, 3, 1), (256, 38, 63, 512, 3, 1), (512, 38, 63, 512, 3, 1), (512, 38, 63, 256, 7, 0)]
    assert split["forward"] == big
    assert split["input_gradient"] == big      # (test_conv_backward_input runs CASES[1:])
    assert split["weight_gradient"] == big[:3]
    # what is left to conv.hip there: the seven small shapes (their split counts: test_split_k_cases)
    rest = [s for s in cases if s not in big]
    assert len(rest) == 7 and {s[4] for s in rest} == {1, 3, 5, 7}
    assert [CP.weight_gradient_plan(s)["kernel"] for s in rest] == ["first"] + ["generic"] * 6


def test_fp64_references_agree_with_the_oracle(O):
    """The numpy references of tests/test_gpu_conv_plans.py against the C oracle (fp64 accumulation, fp32 result): one rounding
    of the result apart at most."""
    rng = np.random.RandomState(5)
    for C_, H, W, O_, k, pad in ((5, 9, 11, 7, 3, 1), (3, 8, 9, 4, 5, 0), (6, 7, 7, 5, 1, 0), (4, 9, 12, 3, 7, 3), (7, 6, 10, 9, 5, 4)):
        Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
        x = rng.randn(C_, H, W).astype(np.float32)
        w = rng.randn(O_, C_, k, k).astype(np.float32)
        b = rng.randn(O_).astype(np.float32)
        g = rng.randn(O_, Ho, Wo).astype(np.float32)
        gw, gb = CP.ref_weight_gradient(x, g, k, pad)
        ogw, ogb = O.conv2d_bwd_weight(x, g, k, k, pad)
        for mine, theirs in ((CP.ref_forward(x, w, b, pad), O.conv2d_fwd(x, w, b, pad)),
                             (CP.ref_input_gradient(g, w, pad, H, W), O.conv2d_bwd_input(g, w, pad, H, W)), (gw, ogw), (gb, ogb)):
            assert mine.dtype == np.float64 and mine.shape == theirs.shape
            assert np.all(np.abs(mine - theirs) <= 2.0 ** -23 * np.abs(mine) + 1e-12)
    x = np.array([[[1.5, -2.0]], [[-4.0, 8.0]]], np.float32)
    assert np.array_equal(CP.activate(x, 0.25, [1.0, 2.0]), np.array([[[1.5, -0.5]], [[-2.0, 16.0]]], np.float32))
    assert np.array_equal(CP.activate(x, None, [0.0, 1.0])[0], np.zeros((1, 2), np.float32))
    assert CP.activate(x, 0.5, None).dtype == np.float32


# ---- the fused pooling epilogue and the pooled first-layer weight gradient (tests/test_gpu_conv_pool.py) -------------------
def test_pool_restatement_at_known_values():
    # block 0 of vgg_small at the benchmark frame (3 -> 64 on 450x800): the first-layer kernel, fused, 25 x 113 tiles
    p = CP.pool_plan(3, 450, 800, 64, 1)
    assert (p["first"], p["fused"], p["blocks"], p["mTiles"]) == (True, True, 25 * 113, 1)
    # the layer named in conv_igemm's comment (200x113): 812 blocks of the fixed tile, a fourth round of 256 where the free tile needs three: refused
    p = CP.pool_plan(128, 113, 200, 256, 1)   # (four M tiles)
    assert (p["blocks"], CP.cdiv(p["blocks"], 256), CP.cdiv(p["free_blocks"], 256), p["tile_refused"], p["fused"]) == (812, 4, 3, True, False)
    # the non-reference backbones of tests/width_plan.py on a 133 x 181 map: the split rule asks for 2 and 3 splits, no fusion
    assert [CP.pool_plan(c, 133, 181, c, 1)["fused"] for c in (48, 96)] == [False, False]
    assert [CP.pool_plan(c, 133, 181, c, 1)["splits_wanted"] for c in (48, 96)] == [2, 3]


def test_pool_cases_reach_what_they_are_listed_for():
    reached = set()
    names = [c["name"] for c in CP.POOL_CASES]
    assert len(names) == len(set(names)) == 16 and set(names) == set(CP.POOL_WANT)
    for c in CP.POOL_CASES:
        C, H, W, M = c["shape"]
        p = CP.pool_plan(C, H, W, M, CP.POOL_PAD)
        labels = CP.pool_labels(p)
        assert c["want"] <= labels, (c["name"], sorted(c["want"] - labels))
        assert (p["fused"], p["blocks"], p["splitK"]) == CP.POOL_WANT[c["name"]], (c["name"], p["fused"], p["blocks"], p["splitK"])
        assert p["fused"] == (p["one_split"] and not p["tile_refused"])
        reached |= labels
    assert CP.POOL_REQUIRED <= reached, sorted(CP.POOL_REQUIRED - reached)
    # the two refusals by the tile rule: 272 blocks of the fixed tile against 208
    for n in ("p_tile_first", "p_tile_generic"):
        p = CP.pool_plan(*CP.find_pool(n)["shape"], CP.POOL_PAD)
        assert (p["blocks"], p["free_blocks"], p["one_split"]) == (272, 208, True)
    # Cin = 48 on a full grid: the split rule would allow 2 splits, 1280 // 660 = 1 leaves one
    p = CP.pool_plan(*CP.find_pool("p_full_grid")["shape"], CP.POOL_PAD)
    assert p["could_split"] and p["splits_wanted"] == 1 and not p["first"]
    p = CP.pool_plan(*CP.find_pool("p_late_record")["shape"], CP.POOL_PAD)
    assert p["grid"] == 16448 > CP.AMAX_MAX_BLOCKS and p["late_record"]
    for n in CP.POOL_VARIANT_BASES:
        assert CP.pool_plan(*CP.find_pool(n)["shape"], CP.POOL_PAD)["fused"]
    assert [CP.pool_plan(*CP.find_pool(n)["shape"], CP.POOL_PAD)["first"] for n in CP.POOL_VARIANT_BASES] == [True, False]
    got = [CP.pool_variant(v) for v in CP.POOL_VARIANTS]
    assert {v["slope"] for v in got} == {0.25, 0.0, -0.5, 1.5, None}
    assert any(v["scale"] for v in got) and any(v["in_act"] for v in got) and any(not v["bias"] for v in got)
    assert any(not v["rec"] for v in got) and CP.pool_variant(None)["rec"]


def test_first_pooled_cases_reach_what_they_are_listed_for():
    reached = set()
    names = [c["name"] for c in CP.FIRST_POOLED_CASES]
    assert len(names) == len(set(names)) == 10
    for c in CP.FIRST_POOLED_CASES:
        p = CP.first_pooled_plan(*c["shape"])
        labels = CP.first_pooled_labels(p)
        assert c["want"] <= labels, (c["name"], sorted(c["want"] - labels))
        reached |= labels
        # what the entry point allocates (conv_wgrad_workspace_bytes) holds the slabs with their extras
        C, H, W, O, pad = c["shape"]
        assert CP.wgrad_plan(C, H, W, O, 3, pad)["kernel"] == "first"
    assert CP.FIRST_POOLED_REQUIRED <= reached, sorted(CP.FIRST_POOLED_REQUIRED - reached)
    for name, mirror in CP.FIRST_POOLED_MIRROR.items():   # the two tables stay comparable
        C, H, W, O, pad = CP.find_pool(name)["shape"]
        assert CP.find(mirror)["shape"] == (C, H, W, O, 3, pad)
        assert CP.first_pooled_plan(C, H, W, O, pad)["nSplit"] == CP.wgrad_plan(C, H, W, O, 3, pad)["nSplit"]
    slabs = {n: CP.first_pooled_plan(*CP.find_pool(n)["shape"]) for n in names}
    assert slabs["fp_127"]["nSplit"] == 127 and slabs["fp_128"]["nSplit"] == 128
    assert (slabs["fp_cap"]["tiles"], slabs["fp_cap"]["nSplit"], slabs["fp_cap"]["tilesPerBlock"]) == (519, 512, 2)
    assert slabs["fp_c3_o64_valid"]["Wo"] == 129 and slabs["fp_wo2"]["Wo"] == 2 and slabs["fp_ho1"]["Ho"] == 1
    assert CP.first_pooled_slope_terms(slabs["fp_cap"]) == 136 and CP.first_pooled_slope_terms(slabs["fp_127"]) == 72
    # the refused shapes: one term of the predicate fails each
    for name, ((C, H, W, O, pad), slope) in CP.FIRST_POOLED_ERRORS.items():
        assert (not CP.first_pooled_eligible(C, O, W + 2 * pad - 2)) == (name != "no_slope"), name
        assert slope == (name != "no_slope")


def test_pool_restatement_in_numpy():
    """pool_act_fp32 / pool_route / ref_pooled_weight_gradient at values that can be checked by hand"""
    x = np.array([[[1.0, 1.0, -2.0], [1.0, 3.0, -8.0], [-4.0, -4.0, 5.0]]], np.float32)
    best, code = CP.pool_act_fp32(x, 0.25, None)
    assert np.array_equal(best, [[[3.0, -0.5], [-1.0, 5.0]]]) and np.array_equal(code, [[[3, 0], [0, 0]]])
    best, code = CP.pool_act_fp32(np.ones((1, 2, 2), np.float32), None, None)   # a four-way tie: the first wins
    assert np.array_equal(code, [[[0]]])
    best, code = CP.pool_act_fp32(x, -0.5, np.array([0.0], np.float32))         # scale 0: ties of +-0 everywhere
    assert not best.any() and not code.any()
    r = CP.pool_route(np.array([[[2.0, 3.0], [5.0, 7.0]]]), np.array([[[3, 0], [0, 0]]], np.uint8), 3, 3)
    assert np.array_equal(r, [[[0, 0, 3.0], [0, 2.0, 0], [5.0, 0, 7.0]]])
    with pytest.raises(AssertionError):
        CP.pool_route(np.ones((1, 2, 2)), np.array([[[0, 1], [0, 0]]], np.uint8), 3, 3)
    inp = np.ones((1, 3, 3), np.float32)
    (gw, gb, gs), (mw, mb, ms) = CP.ref_pooled_weight_gradient(inp, np.array([[[2.0, 3.0], [5.0, 7.0]]]),
                                                                np.array([[[3, 0], [0, 0]]], np.uint8), x, 0.25, 1)
    # g = [[0, 0, .75], [0, 2, 0], [1.25, 0, 7]]
    assert gb[0] == 11.0 and gw[0, 0, 1, 1] == 11.0 and gw[0, 0, 0, 0] == 9.0 and gs == -2.0 * 3.0 + -4.0 * 5.0 and ms == 26.0
    CP.assert_exact_in_fp32(mw, 0.25)
    with pytest.raises(AssertionError):
        CP.assert_exact_in_fp32(2.0 ** 23, 0.25)
