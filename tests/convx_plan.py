"""The case tables of tests/test_gpu_convx_plans.py and a plain restatement of the host-side shape rules of the
split-operand convolutions: csrc/convx.hip (conv_x3: forward and input gradient, 3x3 / 5x5 / 7x7, with its split-K fold)
and csrc/wgradx.hip (conv_wgradx: the 3x3 weight gradient).

As in tests/conv_plan.py, tests/width_plan.py and tests/cnet_plan.py the restatement only LABELS the GPU cases with the
branches they reach, so that tests/test_convx_plan.py can check that the tables still reach every one of them: it is no
evidence that a branch computes the right thing.  The GPU tests against the fp64 references are.

Shapes are written as the operator sees them, (C, H, W, O, k, pad), and a conv_x3 case is written as the FORWARD shape
whose launch it is: the input gradient of conv_plan.mirror(shape) runs the same launch (K channels = C, M = O filters).

The error bound of the split forms is derived at split_bound() below."""
import numpy as np

import conv_plan as CP
import width_plan as WP
from conv_plan import case
from width_plan import cdiv

# ---- convx.hip: conv_x3 -------------------------------------------------------------------------------------------------
CX_CH = 16          # channels per chunk
CX_NTMAX = 128      # pixels per block
CX_OCC = 3          # resident 3x3 blocks per CU
X3_CAP = {3: 16, 5: 24, 7: 24}


def cx_pp(k):
    """patch positions a block can stage"""
    return 204 if k == 3 else 240 if k == 5 else 308


def x3_choose_tile(Ho, Wo, k):
    """convx.hip x3_choose_tile -> (TH, TW, cut): tile widths are multiples of 4 where the map's width is one; cut = the
    patch plane, not the 128 pixels or the map, limits the height of the chosen tile"""
    mult = 4 if Wo % 4 == 0 else 1
    best, bth, btw, bcut = -1, 1, 1, False
    for tw in range(1, min(Wo, CX_NTMAX) + 1):
        if (tw < 8 and Wo >= 8) or tw % mult:
            continue
        th0 = th = min(CX_NTMAX // tw, Ho)
        while th > 1 and (th + k - 1) * (tw + k - 1) > cx_pp(k):
            th -= 1
        if th < 1 or (th + k - 1) * (tw + k - 1) > cx_pp(k):
            continue
        tiles = cdiv(Ho, th) * cdiv(Wo, tw)
        cost = tiles * CX_NTMAX * 64 + tiles * (th + k - 1) * (tw + k - 1)
        if best < 0 or cost < best or (cost == best and tw > btw):
            best, bth, btw, bcut = cost, th, tw, th < th0
    return bth, btw, bcut


def conv_x3_bm(M, Ho, Wo, k):
    """convx.hip conv_x3_bm -> (filters per block, why)"""
    bm = WP.conv_x3_bm(M, k)          # the M % 128 part
    if bm == 64:
        return 64, "indivisible"
    if bm == 128:
        return 128, "k"
    TH, TW, _ = x3_choose_tile(Ho, Wo, k)
    tiles = cdiv(Ho, TH) * cdiv(Wo, TW)
    b128, b64 = tiles * (M // 128), tiles * (M // 64)
    if b128 < 512 and 512 <= b64 <= 256 * CX_OCC:
        return 64, "fill_rule"
    return 128, "default"


def x3_plan(shape, out_aligned=True, post=False, post_aligned=True):
    """convx.hip conv_x3 for the launch of forward shape `shape` (or of the input gradient of its mirror).
    out_aligned: the destination tensor is 16-byte aligned; post: the launch carries the fused activation backward
    (X3PostAct), post_aligned: its x is 16-byte aligned."""
    Cin, H, W, M, k, pad = shape
    assert WP.conv_x3_eligible(Cin, M, k), shape
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    assert Ho > 0 and Wo > 0
    TH, TW, cut = x3_choose_tile(Ho, Wo, k)
    tilesX, tilesY = cdiv(Wo, TW), cdiv(Ho, TH)
    bm, why = conv_x3_bm(M, Ho, Wo, k)
    mTiles, nChunks = M // bm, Cin // CX_CH
    blocks = tilesX * tilesY * mTiles
    min_chunks = 4 if k == 3 else 1          # 36 stages of a 3x3; one 25- / 49-stage chunk of a 5x5 / 7x7
    slots = 256 * (CX_OCC if k == 3 else 2)
    estimate = min(min(max(1, slots // blocks), X3_CAP[k]), max(1, nChunks // min_chunks))
    cps = cdiv(nChunks, estimate)
    splitK = cdiv(nChunks, cps)
    slab = splitK > 1
    # the tile epilogue stores into the slab workspace (an allocation of its own: aligned) when K is split
    wide = Wo % 4 == 0 and TW % 4 == 0 and (slab or out_aligned) and (not post or post_aligned)
    vec = None
    if slab:
        al = out_aligned and (not post or post_aligned)
        hw = Ho * Wo
        vec = 4 if al and hw % 4 == 0 else 2 if al and hw % 2 == 0 else 1
    return dict(k=k, Cin=Cin, M=M, Ho=Ho, Wo=Wo, TH=TH, TW=TW, cut=cut, tilesX=tilesX, tilesY=tilesY, bm=bm, why=why,
                mTiles=mTiles, nChunks=nChunks, blocks=blocks, estimate=estimate, chunksPerSplit=cps, splitK=splitK,
                lastSplitChunks=nChunks - (splitK - 1) * cps, wide=wide, vec=vec, out_aligned=out_aligned, post=post,
                post_aligned=post_aligned, where="fold" if slab else "tile", K=Cin * k * k)


def x3_labels(p, bias=False, add=False, act=None, post_scale=None):
    """labels of one conv_x3 launch.  bias / add (OUT_ADD) / post-activation are applied where p["where"] says: in the tile
    epilogue of a one-slab launch, in the fold of a split one.  act: None, "slope", "scale", "both" (the staging loader's
    fused input activation); post_scale: None (no post-activation), True / False (X3PostAct with / without a scale)."""
    assert (post_scale is not None) == p["post"]
    L = {"k%d" % p["k"]}
    L.add({"indivisible": "bm64_indivisible", "fill_rule": "bm64_fill_rule"}.get(p["why"], "bm128"))
    if p["nChunks"] == 1:
        L.add("one_chunk")
    if p["tilesX"] * p["tilesY"] == 1:
        L.add("tile_whole_map")
    if p["Ho"] == 1 and p["Wo"] == 1:
        L.add("map_1x1")
    if p["Wo"] % p["TW"] and p["tilesX"] > 1:
        L.add("ragged_x")
    if p["Ho"] % p["TH"] and p["tilesY"] > 1:
        L.add("ragged_y")
    if p["Wo"] < 8:
        L.add("wo_lt_8")
    if p["cut"]:
        L.add("th_cut_by_patch_plane")
    if p["wide"]:
        L.add("wide")
    elif p["Wo"] % 4 or p["TW"] % 4:
        L.add("narrow_width")
    else:
        L.add("narrow_misaligned")
    if p["splitK"] == 1:
        L.add("one_slab")
        if add:
            L.add("epilogue_add")
    else:
        L.add("splitk")
        if p["lastSplitChunks"] < p["chunksPerSplit"]:
            L.add("last_split_short")
        if p["splitK"] < p["estimate"]:
            L.add("splits_recomputed")
        if p["splitK"] == X3_CAP[p["k"]]:
            L.add("splitk_cap%d" % X3_CAP[p["k"]])
        L.add("fold_vec%d" % p["vec"])
        if not (p["out_aligned"] and p["post_aligned"]):
            L.add("fold_misaligned")
        L.add("fold_bias" if bias else "fold_no_bias")
        if add:
            L.add("fold_add")
    if act is not None:
        L.add("act_" + act)
        L.add("act_%s_bm%d" % (act, p["bm"]))
    if p["post"]:
        L.add("post_scale" if post_scale else "post_no_scale")
        if p["where"] == "fold":
            L.add("post_fold")
            L.add("post_fold_vec%d" % p["vec"])
        else:
            L.add("post_inline_bm%d" % p["bm"])
            L.add("post_inline_wide" if p["wide"] else "post_inline_narrow")
    return L


# ---- wgradx.hip: conv_wgradx --------------------------------------------------------------------------------------------
WX_TH, WX_TW = 4, 16


def wgradx_plan(shape):
    """wgradx.hip wgradx_plan and the kernel's division-free tile walk: block `split` takes the pixel tiles split + i nSplit"""
    Cin, H, W, O, k, pad = shape
    assert WP.conv_wgradx_eligible(Cin, O, k), shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    assert Ho > 0 and Wo > 0
    tilesX, tilesY = cdiv(Wo, WX_TW), cdiv(Ho, WX_TH)
    oTiles, cTiles = O // 64, Cin // 64
    base, npix = oTiles * cTiles, tilesX * tilesY
    nSplit = max(1, min(npix, 256 // base))
    nT = [(npix - s + nSplit - 1) // nSplit for s in range(nSplit)]
    adv_y, adv_x = nSplit // tilesX, nSplit % tilesX
    wraps = False
    for s in range(nSplit):   # the walk of load_origin, checked against the division it replaces
        ty, tx = s // tilesX, s % tilesX
        for i in range(nT[s]):
            assert ty * tilesX + tx == s + i * nSplit
            if i + 1 < nT[s]:
                tx, ty = tx + adv_x, ty + adv_y
                if tx >= tilesX:
                    tx, ty, wraps = tx - tilesX, ty + 1, True
    return dict(Cin=Cin, O=O, H=H, W=W, Ho=Ho, Wo=Wo, pad=pad, tilesX=tilesX, tilesY=tilesY, oTiles=oTiles, cTiles=cTiles,
                npix=npix, nSplit=nSplit, nT=nT, adv_x=adv_x, adv_y=adv_y, wraps=wraps, K=Ho * Wo,
                slab_floats=nSplit * 9 * O * Cin)


def wgradx_loader(p, aligned=True, slack=True):
    """wgradx.hip launch_wgradx -> VEC.  aligned: both tensors start on 16 bytes; slack: both allocations extend at least 12
    bytes past the tensors' ends (readable_past_end)"""
    if p["pad"] == 1 and p["W"] % 4 == 0 and aligned:
        return 1
    if p["pad"] == 1 and slack:
        return 2
    return 0


def wgradx_labels(p, act=None, aligned=True, slack=True, gbias=True):
    vec = wgradx_loader(p, aligned, slack)
    L = set()
    if p["npix"] == 1:
        L.add("wg_one_tile")
    for n in set(p["nT"]):
        L.add("wg_nt%d" % n if n < 4 else "wg_nt4plus")
    uneven = len(set(p["nT"])) > 1
    if uneven:
        L.add("wg_uneven")
    if p["adv_x"]:
        L.add("wg_advx_nonzero")
    if p["wraps"]:
        L.add("wg_walk_wraps")
    if vec:
        L.add("wg_vec%d" % vec)
    else:
        L.add("wg_vec0_pad0" if p["pad"] != 1 else "wg_vec0_no_slack")
    if act is not None:
        L.add("wg_act_" + act)
        L.add("wg_act_%s_vec%d" % (act, vec))
    if gbias:
        L.add("wg_gbias")
        if uneven:
            L.add("wg_gbias_uneven")
        if vec == 2 and p["Wo"] % 4:
            L.add("wg_gbias_row_overhang")
    if p["Ho"] % WX_TH or p["Wo"] % WX_TW:
        L.add("wg_partial_tile")
    return L


# ---- case tables: conv_x3 -----------------------------------------------------------------------------------------------
# Every case runs the forward (with a bias) and the input gradient of its mirror (accumulate 0 and 1), in both operand forms.
X3_CASES = [
    # one output pixel
    case("pixel_k3", (16, 3, 3, 64, 3, 0), "k3", "map_1x1", "one_chunk", "bm64_indivisible", "tile_whole_map", "wo_lt_8"),
    case("pixel_k5", (16, 5, 5, 128, 5, 0), "k5", "map_1x1", "one_chunk", "bm128"),
    case("pixel_k7", (16, 7, 7, 128, 7, 0), "k7", "map_1x1", "one_chunk"),
    # 64-filter blocks through the fill rule of conv_x3_bm: 256 tiles x 128 filters, 128 tiles x 256 filters
    case("fill_128", (16, 128, 256, 128, 3, 1), "bm64_fill_rule", "one_chunk", "wide", "one_slab"),
    case("fill_256", (16, 64, 256, 256, 3, 1), "bm64_fill_rule", "one_chunk", "wide"),
    # one slab: ragged tiles, both block sizes, both epilogues
    case("ragged_bm128", (32, 19, 21, 128, 3, 1), "bm128", "ragged_x", "ragged_y", "narrow_width", "one_slab"),
    case("ragged_y_bm64", (32, 30, 8, 64, 3, 1), "bm64_indivisible", "ragged_y", "wide", "one_slab"),
    case("ragged_x_wide", (32, 6, 28, 128, 3, 1), "bm128", "ragged_x", "wide", "one_slab"),
    case("ragged_x_wide_bm64", (48, 5, 36, 64, 3, 1), "bm64_indivisible", "ragged_x", "wide", "one_slab"),
    case("two_tiles_bm128", (32, 20, 12, 128, 3, 1), "bm128", "wide", "one_slab"),
    case("two_tiles_bm64", (64, 13, 18, 64, 3, 1), "bm64_indivisible", "narrow_width", "one_slab"),
    case("two_slabs_k5", (32, 7, 9, 128, 5, 0), "k5", "splitk", "tile_whole_map", "wo_lt_8"),
    case("slab_k7", (16, 13, 16, 128, 7, 0), "k7", "one_slab", "one_chunk", "tile_whole_map"),
    # split K
    case("short_last", (144, 12, 16, 128, 3, 1), "splitk", "last_split_short", "wide", "fold_vec4"),
    case("short_last_vec2", (208, 9, 14, 64, 3, 1), "splitk", "last_split_short", "narrow_width", "fold_vec2", "bm64_indivisible"),
    case("short_last_vec2_bm128", (144, 10, 13, 128, 3, 1), "splitk", "last_split_short", "fold_vec2", "bm128"),
    case("scalar_fold", (128, 13, 15, 128, 3, 1), "splitk", "fold_vec1", "narrow_width", "ragged_x"),
    case("cap16", (1024, 8, 8, 128, 3, 1), "splitk_cap16", "wide", "fold_vec4", "tile_whole_map"),
    case("cap16_bm64", (1024, 5, 7, 64, 3, 1), "splitk_cap16", "fold_vec1", "wo_lt_8", "bm64_indivisible"),
    case("cap24", (384, 9, 12, 128, 7, 0), "k7", "splitk_cap24", "fold_vec2", "wo_lt_8"),
    case("cap24_wide", (384, 10, 14, 128, 7, 0), "k7", "splitk_cap24", "fold_vec4", "wide"),
    case("recomputed_k3", (480, 8, 8, 64, 3, 1), "splits_recomputed", "bm64_indivisible", "wide"),
    case("nine_slabs_k5", (144, 9, 12, 128, 5, 0), "k5", "splitk", "fold_vec4", "wide"),
    case("recomputed_k5", (416, 9, 12, 128, 5, 0), "k5", "splits_recomputed", "fold_vec4", "wide"),
    case("cut_k3", (16, 50, 3, 64, 3, 1), "k3", "th_cut_by_patch_plane", "ragged_y", "wo_lt_8", "one_chunk"),
    case("cut_k5", (64, 19, 22, 128, 5, 0), "k5", "th_cut_by_patch_plane", "splitk", "ragged_y"),
    case("cut_k7", (32, 25, 26, 128, 7, 0), "k7", "th_cut_by_patch_plane", "splitk", "ragged_y", "wide"),
]
# (with k = 3 only a tall map narrower than 8 pixels gets a tile that the 204-position patch plane cuts: 38 x 3 here)

# the forward without a bias (the fold and the tile epilogue then skip the bias load)
X3_NO_BIAS = ["short_last", "scalar_fold", "cap24", "cut_k5", "ragged_bm128", "fill_256"]
# destination 4 bytes into a larger buffer: forward, and the input gradient with accumulate 0 and 1
X3_MISALIGNED = ["two_tiles_bm128", "ragged_y_bm64", "ragged_x_wide", "short_last", "cap24_wide", "recomputed_k3"]
# fused input activation of the forward (3x3 only): (case, mode)
ACT_MODES = CP.ACT_MODES
X3_ACT = [(n, m) for n in ("ragged_bm128", "short_last", "ragged_y_bm64", "recomputed_k3") for m in ACT_MODES]
# fused activation backward of the input gradient (frcnn_conv2d_backward_input_rec): (case, with a scale, post_x misaligned)
X3_POST = [
    ("two_tiles_bm128", True, False), ("ragged_x_wide", False, False),            # inline, 128 filters, wide
    ("ragged_bm128", False, False),                                              # ... narrow by the width
    ("two_tiles_bm128", False, True), ("ragged_y_bm64", True, True),              # ... narrow by a misaligned x
    ("ragged_y_bm64", False, False), ("ragged_x_wide_bm64", True, False),         # inline, 64 filters, wide
    ("two_tiles_bm64", True, False),                                             # ... narrow
    ("short_last", True, False), ("recomputed_k3", False, False),                 # fold, four pixels per thread
    ("short_last_vec2", False, False), ("short_last_vec2_bm128", True, False),    # fold, two
    ("scalar_fold", True, False), ("cap16_bm64", False, False),                   # fold, one
    ("short_last", False, True),                                                 # fold, one by a misaligned x
]


def find_x3(name):
    for c in X3_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def x3_runs():
    """every conv_x3 launch of tests/test_gpu_convx_plans.py: dicts of role, case name, shape and the options its labels
    depend on (x3_labels_of_run)"""
    runs = []
    for c in X3_CASES:
        runs.append(dict(role="forward", name=c["name"], shape=c["shape"], bias=True))
        for acc in (0, 1):
            runs.append(dict(role="input_gradient", name=c["name"], shape=c["shape"], add=bool(acc)))
    for n in X3_NO_BIAS:
        runs.append(dict(role="forward", name=n, shape=find_x3(n)["shape"], bias=False))
    for n in X3_MISALIGNED:
        runs.append(dict(role="forward", name=n, shape=find_x3(n)["shape"], bias=True, out_aligned=False))
        for acc in (0, 1):
            runs.append(dict(role="input_gradient", name=n, shape=find_x3(n)["shape"], add=bool(acc), out_aligned=False))
    for n, m in X3_ACT:
        runs.append(dict(role="forward", name=n, shape=find_x3(n)["shape"], bias=True, act=m))
    for n, sc, mis in X3_POST:
        runs.append(dict(role="post", name=n, shape=find_x3(n)["shape"], post_scale=sc, post_aligned=not mis))
    return runs


def x3_plan_of_run(r):
    return x3_plan(r["shape"], out_aligned=r.get("out_aligned", True), post=r["role"] == "post",
                   post_aligned=r.get("post_aligned", True))


def x3_labels_of_run(r):
    return x3_labels(x3_plan_of_run(r), bias=r.get("bias", False), add=r.get("add", False), act=r.get("act"),
                     post_scale=r.get("post_scale"))


X3_REQUIRED = {
    "k3", "k5", "k7", "bm128", "bm64_indivisible", "bm64_fill_rule", "one_chunk", "tile_whole_map", "map_1x1", "ragged_x",
    "ragged_y", "wo_lt_8", "th_cut_by_patch_plane", "wide", "narrow_width", "narrow_misaligned", "one_slab", "splitk",
    "last_split_short", "splits_recomputed", "splitk_cap16", "splitk_cap24", "fold_vec4", "fold_vec2", "fold_vec1",
    "fold_misaligned", "fold_bias", "fold_no_bias", "fold_add", "epilogue_add",
    "act_slope", "act_scale", "act_both", "act_slope_bm128", "act_scale_bm128", "act_both_bm128", "act_slope_bm64",
    "act_scale_bm64", "act_both_bm64",
    "post_inline_bm128", "post_inline_bm64", "post_inline_narrow", "post_inline_wide", "post_fold", "post_fold_vec4",
    "post_fold_vec2", "post_fold_vec1", "post_scale", "post_no_scale",
}

# ---- case tables: conv_wgradx ---------------------------------------------------------------------------------------------
# place: where the two tensors lie.  "slack": each at the start of an allocation at least 16 bytes longer than the tensor
# (aligned); "exact": each ends where its allocation ends (aligned); "offset": each 4 bytes into an allocation with slack.
WG_PLACES = {"slack": dict(aligned=True, slack=True), "exact": dict(aligned=True, slack=False),
             "offset": dict(aligned=False, slack=True)}


def wcase(name, shape, place, *want):
    c = case(name, shape, *want)
    c["place"] = place
    return c


WG_CASES = [
    wcase("tile", (64, 4, 16, 64, 3, 1), "slack", "wg_one_tile", "wg_nt1", "wg_vec1"),
    wcase("tile_pad0", (64, 5, 17, 64, 3, 0), "slack", "wg_one_tile", "wg_nt1", "wg_vec0_pad0", "wg_partial_tile"),
    wcase("nt3_nt2", (512, 12, 40, 512, 3, 1), "slack", "wg_nt3", "wg_nt2", "wg_uneven", "wg_advx_nonzero", "wg_walk_wraps",
          "wg_vec1", "wg_gbias_uneven"),
    wcase("advx2", (256, 16, 40, 512, 3, 1), "slack", "wg_nt1", "wg_nt2", "wg_uneven", "wg_advx_nonzero", "wg_walk_wraps", "wg_vec1"),
    wcase("advx4", (128, 60, 80, 128, 3, 1), "slack", "wg_advx_nonzero", "wg_walk_wraps", "wg_uneven", "wg_vec1"),
    wcase("nt5_nt4", (512, 24, 48, 512, 3, 1), "slack", "wg_nt4plus", "wg_uneven", "wg_vec1", "wg_walk_wraps"),
    wcase("nt3_odd", (512, 16, 35, 512, 3, 1), "slack", "wg_nt3", "wg_vec2", "wg_gbias_row_overhang", "wg_walk_wraps"),
    wcase("nt5_nt4_odd", (512, 22, 45, 512, 3, 1), "slack", "wg_nt4plus", "wg_vec2", "wg_gbias_row_overhang", "wg_gbias_uneven"),
    wcase("nt3_nt2_odd", (256, 18, 50, 512, 3, 1), "slack", "wg_nt3", "wg_nt2", "wg_vec2", "wg_gbias_row_overhang"),
    wcase("small_odd", (64, 9, 11, 64, 3, 1), "slack", "wg_nt1", "wg_vec2", "wg_gbias_row_overhang", "wg_partial_tile"),
    wcase("advx2_offset", (256, 16, 40, 512, 3, 1), "offset", "wg_vec2", "wg_advx_nonzero", "wg_uneven"),
    wcase("pad0", (64, 10, 20, 64, 3, 0), "slack", "wg_vec0_pad0", "wg_partial_tile"),
    wcase("pad0_odd", (128, 14, 37, 64, 3, 0), "slack", "wg_vec0_pad0", "wg_partial_tile"),
    wcase("small_odd_exact", (64, 9, 11, 64, 3, 1), "exact", "wg_vec0_no_slack", "wg_nt1"),
    wcase("nt3_nt2_exact", (512, 12, 34, 512, 3, 1), "exact", "wg_vec0_no_slack", "wg_nt3", "wg_nt2", "wg_walk_wraps"),
]
# fused input activation of the weight gradient on each loader: (case, mode)
WG_ACT = [("small_odd", m) for m in ACT_MODES] + [("tile", m) for m in ACT_MODES] + [("pad0", m) for m in ACT_MODES] + [
    ("nt3_nt2", "both"), ("nt3_odd", "both"), ("small_odd_exact", "both")]


def find_wg(name):
    for c in WG_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def wg_runs():
    runs = [dict(name=c["name"], shape=c["shape"], place=c["place"], act=None) for c in WG_CASES]
    runs += [dict(name=n, shape=find_wg(n)["shape"], place=find_wg(n)["place"], act=m) for n, m in WG_ACT]
    return runs


def wg_labels_of_run(r):
    return wgradx_labels(wgradx_plan(r["shape"]), act=r["act"], **WG_PLACES[r["place"]])


WG_REQUIRED = {
    "wg_one_tile", "wg_nt1", "wg_nt2", "wg_nt3", "wg_nt4plus", "wg_uneven", "wg_advx_nonzero", "wg_walk_wraps", "wg_vec1",
    "wg_vec2", "wg_vec0_pad0", "wg_vec0_no_slack", "wg_act_slope", "wg_act_scale", "wg_act_both", "wg_act_both_vec1",
    "wg_act_both_vec2", "wg_act_both_vec0", "wg_gbias", "wg_gbias_uneven", "wg_gbias_row_overhang", "wg_partial_tile",
}
REQUIRED = X3_REQUIRED | WG_REQUIRED
# labels that fewer than two shapes can reach within the size limit of the tables, with the reason: none.
FEWER_THAN_TWO = {}


# ---- the error bound of the split forms ------------------------------------------------------------------------------------
# A result of convx.hip / wgradx.hip is an fp32 sum, taken in any order, of EXACT partial products of 16-bit planes:
#   three bf16 planes (convx.hip's header):  x = h + m + l + eps, |eps| <= 2^-26 |x|; six of the nine plane products are
#       kept, the dropped m l', l m', l l' are <= 2^-25 |x y| together.  So the kept products of one fp32 product miss it by
#       at most (2^-26 + 2^-26 + 2^-52 + 2^-25) |x y| <= 2^-24 (1 + 2^-20) |x y|.
#   two fp16 planes (convx.hip at split8h):  X = x 2^e = h + l + eps with e putting the tensor's largest magnitude A into
#       [2^14, 2^15) -- [2^13, 2^14) under a dropout scale --, |eps| <= 2^-22 |X| where the residual is a normal fp16 number
#       and <= 2^-25 (half a subnormal step) where it is not: in the tensor's own units |eps| <= 2^-22 |x| + 2^-38 A, as
#       _tap_equal of tests/test_gpu_convx.py states it.  h h' + h l' + l h' are kept; the dropped l l' is at most
#       (2^-11 (1 + 2^-11) |x| + 2^-38 A)(the same of y).
# so with d(x) = 2^-22 |x| + 2^-38 A_x and r(x) = 2^-11 (1 + 2^-11) |x| + 2^-38 A_x the kept products of x y miss it by
#       d(x) |y| + |x| d(y) + d(x) d(y) + r(x) r(y)
# (representation_bound: the same convolution taken on these magnitudes).  tests/test_convx_plan.py emulates both splits in
# numpy, sums the kept products in fp64 and checks that share for every case.
# On top comes the fp32 accumulation of the n = P K kept products (P = 6 or 3 per fp32 product, K the length of the dot
# product) and of the S slabs, a bias or an accumulating destination, in any order: (n + S + 2) 2^-24 mag to first order
# (conv_plan.rounding_bound), mag = the same operation on magnitudes.  The kept products' magnitudes sum to at most
# (1 + 2^-7) |x y| (|h| <= (1 + 2^-8) |x|, |m| <= 2^-8 |x|, |l| <= 2^-16 |x|), hence the factor MAG_SLACK.
# The fp16 form undoes its scaling by two powers of two, which is exact.
PRODUCTS = {0: 6, 1: 3}          # kept plane products per fp32 product, by option x3_f16
MAG_SLACK = 1.0 + 2.0 ** -7


def _amax(a):
    return float(np.abs(np.asarray(a, np.float64)).max()) if np.size(a) else 0.0


def representation_terms(a, f16, amax=None):
    """-> (d, r) of the comment above for operand a (fp32 values as the kernel splits them).  amax: the magnitude the fp16
    form scales by, where it is not the operand's own largest (a fused activation: the raw tensor's, times max(1, |slope|))"""
    m = np.abs(np.asarray(a, np.float64))
    if not f16:
        return 2.0 ** -26 * m, 2.0 ** -9 * (1 + 2.0 ** -8) * m
    A = _amax(a) if amax is None else float(amax)
    nz = (m > 0)   # an exact zero (padding, a dropped channel) has planes of zero
    return (2.0 ** -22 * m + 2.0 ** -38 * A) * nz, (2.0 ** -11 * (1 + 2.0 ** -11) * m + 2.0 ** -38 * A) * nz


def representation_bound(op, a, b, f16, amax_a=None, amax_b=None):
    """the share of the operands' representation in the bound: op(a', b') is the bilinear operation on magnitudes (for
    instance lambda x, w: ref_forward(x, w, None, pad))"""
    ma, mb = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    da, ra = representation_terms(a, f16, amax_a)
    db, rb = representation_terms(b, f16, amax_b)
    if not f16:   # d is a multiple of the magnitude; the three dropped products m l', l m', l l' are <= 2^-25 |x y| together
        return (2.0 ** -26 + 2.0 ** -26 + 2.0 ** -52 + 2.0 ** -25) * op(ma, mb)
    return op(da, mb + db) + op(ma, db) + op(ra, rb)


def split_bound(n_products, S, mag, rep, extra=2):
    """n_products = P K kept partial products, S slabs, `extra` further roundings (bias / destination; the activation backward
    adds two), mag on magnitudes, rep = representation_bound(...)"""
    return (n_products + S + extra) * CP.U * MAG_SLACK * np.asarray(mag, np.float64) + rep


# ---- the two splits, emulated (tests/test_convx_plan.py: the representation share alone) -------------------------------------
def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)


def planes_bf16(a):
    a = np.asarray(a, np.float32)
    h = bf16_round(a)
    r = (a - h).astype(np.float32)
    m = bf16_round(r)
    l = bf16_round((r - m).astype(np.float32))
    return [h.astype(np.float64), m.astype(np.float64), l.astype(np.float64)]


def f16_exponent(amax, top=14):
    """convx.hip x16_exp"""
    if not np.isfinite(amax) or amax < 2.0 ** -126:
        return 0
    e = top - int(np.floor(np.log2(float(amax))))
    return max(-100, min(100, e))


def planes_f16(a, amax=None, top=14):
    """-> ([h, l] of a 2^e, e)"""
    a = np.asarray(a, np.float32)
    e = f16_exponent(_amax(a) if amax is None else amax, top)
    X = (a * np.float32(2.0 ** e)).astype(np.float32)
    h = X.astype(np.float16)
    l = (X - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return [h.astype(np.float64), l.astype(np.float64)], e


def emulate_split(op, a, b, f16, amax_a=None, amax_b=None, top_a=14, top_b=14):
    """op on the kept plane products, summed in fp64.  op is bilinear, so the kept products are all of them less the dropped:
    (h + l) (h' + l') - l l' with two planes, (h + m + l) (h' + m' + l') - (m + l) l' - l m' with three"""
    if f16:
        (ha, la), ea = planes_f16(a, amax_a, top_a)
        (hb, lb), eb = planes_f16(b, amax_b, top_b)
        return (op(ha + la, hb + lb) - op(la, lb)) * 2.0 ** -(ea + eb)
    ha, ma, la = planes_bf16(a)
    hb, mb, lb = planes_bf16(b)
    return op(ha + ma + la, hb + mb + lb) - op(ma + la, lb) - op(la, mb)


def representation_share(op, a, b, f16, what, amax_a=None, amax_b=None, top_a=14):
    """asserts that the emulated split misses op(a, b) by no more than representation_bound; -> the largest distance / share"""
    want = op(np.asarray(a, np.float64), np.asarray(b, np.float64))
    got = emulate_split(op, a, b, f16, amax_a=amax_a, amax_b=amax_b, top_a=top_a)
    rep = representation_bound(op, a, b, f16, amax_a=amax_a, amax_b=amax_b)
    err = np.abs(got - want)
    worst = float((err / np.maximum(rep, 1e-300)).max())
    assert np.all(err <= rep), "%s: the kept plane products miss the product by %.3f times the representation share" % (what, worst)
    return worst
