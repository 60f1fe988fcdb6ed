"""The case tables of tests/test_gpu_conv_plans.py and a plain restatement of the host-side shape rules of the fp32
matrix-core convolutions (csrc/conv.hip: conv_igemm, conv_wgrad and their split-K folds), plus the rules that decide
whether an operator-level call reaches them at all (tests/width_plan.py: the split forms of convx.hip / wgradx.hip).

As in tests/width_plan.py and tests/cnet_plan.py the restatement only LABELS the GPU cases with the branches they
reach, so that tests/test_conv_plan.py can check that the tables still reach every one of them: it is no evidence that
a branch computes the right thing.  The GPU tests against the fp64 references are.

Shapes are written as the operator sees them: (C, H, W, O, k, pad) = input channels, input map, filters, kernel, padding.
The input gradient of such a convolution is conv_igemm run on the gradient map with the roles of C and O exchanged
(K channels = O, M = C, pad' = k - 1 - pad); mirror() turns a forward shape into the input-gradient shape that takes
exactly the same launch plan, so ONE table serves both roles.

The tables of tests/test_gpu_conv_pool.py live here as well: pool_plan restates when conv_igemm takes a block's max pool into
its epilogue (POOL_CASES, shapes (C, H, W, M) at pad 1), first_pooled_plan the first layer's weight gradient from the pooled
map's gradient (FIRST_POOLED_CASES, shapes (C, H, W, O, pad)), with the float32 / fp64 restatements those tests compare with."""
import numpy as np

import width_plan as WP
from width_plan import cdiv


def case(name, shape, *want):
    """an entry of a case table: the labels in `want` are what the case is listed for"""
    return dict(name=name, shape=tuple(shape), want=set(want))

# ---- conv.hip: forward / input gradient -------------------------------------------------------------------------------
IG_NTW = 2          # 32-pixel tiles per wave along N: an output tile has at most 64 * IG_NTW = 128 pixels
IG_BPC = 5          # resident blocks per CU of the spatial kernels
IG_MAXIT = 4        # patch plane <= 256 * IG_MAXIT positions
IG_MAX_SPLITS = 24


def conv_cc(k):
    """channels per K chunk"""
    return 32 if k == 1 else (8 if k == 3 else 2)


def conv_mpad(M):
    return 64 if M <= 64 else cdiv(M, 128) * 128


def choose_tile(Ho, Wo, k, maxNT=64 * IG_NTW):
    """conv.hip choose_tile: the output tile (TH x TW <= maxNT pixels, patch plane <= 1024) of the least cost"""
    best, bth, btw = -1, 1, 1
    for tw in range(1, min(Wo, maxNT) + 1):
        if tw < 8 and Wo >= 8:
            continue
        th = min(maxNT // tw, Ho)
        if th < 1:
            continue
        if (th + k - 1) * (tw + k - 1) > 256 * IG_MAXIT:
            continue
        tiles = cdiv(Ho, th) * cdiv(Wo, tw)
        cost = tiles * maxNT * 64 + tiles * (th + k - 1) * (tw + k - 1)
        if best < 0 or cost < best or (cost == best and tw > btw):
            best, bth, btw = cost, th, tw
    return bth, btw


def igemm_plan(Cin, H, W, M, k, pad, act=False):
    """conv.hip conv_igemm (no fused pool): Cin K channels on an H x W map, M output rows.  act: in_slope or in_scale given."""
    assert k in (1, 3, 5, 7)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    assert Ho > 0 and Wo > 0
    Mpad = conv_mpad(M)
    BM = 64 if (Mpad == 64 or k > 1) else 128
    cc = conv_cc(k)
    nChunks = cdiv(Cin, cc)
    mTiles = Mpad // BM
    slots = 256 * IG_BPC if k > 1 else 768
    minChunks = 2 if k == 1 else max(1, cdiv(200, cc * k * k))
    TH, TW = choose_tile(Ho, Wo, k)
    tilesX, tilesY = cdiv(Wo, TW), cdiv(Ho, TH)
    blocks = tilesX * tilesY * mTiles
    splits = min(min(max(1, slots // blocks), IG_MAX_SPLITS), max(1, nChunks // minChunks))
    cps = cdiv(nChunks, splits)
    splitK = cdiv(nChunks, cps)
    first = k == 3 and Cin <= 4
    if first:   # a 4-channel chunk, one split
        cc, nChunks, cps, splitK = 4, 1, 1, 1
    plane = (TH + k - 1) * (TW + k - 1)
    NIT = 1 if plane <= 256 else (2 if plane <= 512 else 4)
    if act:
        loader = "act"
    else:
        loader = "dma" if k > 1 else "plain"   # (k == 1: the double-buffered kernel stages through registers)
    return dict(k=k, Cin=Cin, M=M, Ho=Ho, Wo=Wo, Mpad=Mpad, BM=BM, cc=cc, nChunks=nChunks, mTiles=mTiles, TH=TH, TW=TW,
                tilesX=tilesX, tilesY=tilesY, blocks=blocks, plane=plane, NIT=NIT, first=first, loader=loader,
                splitK=splitK, chunksPerSplit=cps, lastSplitChunks=nChunks - (splitK - 1) * cps,
                lastChunkChannels=Cin - (nChunks - 1) * cc, fold="splitk_reduce" if splitK > 1 else None,
                K=Cin * k * k)


def mirror(shape):
    """forward shape -> the input-gradient shape (same notation) whose conv_igemm launch has the same plan"""
    C, H, W, O, k, pad = shape
    return (O, H + 2 * pad - k + 1, W + 2 * pad - k + 1, C, k, k - 1 - pad)


def forward_plan(shape, act=False):
    C, H, W, O, k, pad = shape
    return igemm_plan(C, H, W, O, k, pad, act)


def input_gradient_plan(shape):
    C, H, W, O, k, pad = shape
    return igemm_plan(O, H + 2 * pad - k + 1, W + 2 * pad - k + 1, C, k, k - 1 - pad)


def igemm_labels(p):
    L = {"k%d" % p["k"], "nit%d" % p["NIT"], "bm%d" % p["BM"], "mpad%d" % min(p["Mpad"], 256), "loader_" + p["loader"]}
    if p["first"]:
        L.add("first_layer")
    if p["splitK"] > 1:
        L.add("splitk")
        if p["splitK"] == IG_MAX_SPLITS:
            L.add("splitk_cap")
        if p["lastSplitChunks"] == p["chunksPerSplit"]:
            L.add("splits_even")
        else:
            L.add("last_split_short")
            if p["lastSplitChunks"] == 1:
                L.add("last_split_one_chunk")
    else:
        L.add("one_slab")
    if p["lastChunkChannels"] < p["cc"]:
        L.add("last_chunk_partial")
    if p["k"] >= 5 and p["Cin"] % 2:
        L.add("zero_half_pair")
    if p["M"] < 18:
        L.add("m_below_18")
    if p["Ho"] == 1 and p["Wo"] == 1:
        L.add("one_pixel")
    elif p["Ho"] == 1:
        L.add("one_row")
    if p["Wo"] < 8:
        L.add("tw_below_8")
    if p["Wo"] % p["TW"] and p["tilesX"] > 1:
        L.add("ragged_x")
    if p["Ho"] % p["TH"] and p["tilesY"] > 1:
        L.add("ragged_y")
    if p["blocks"] > 1:
        L.add("many_blocks")
    return L


# ---- conv.hip: the 2x2 max pool in conv_igemm's epilogue (frcnn_conv2d_forward_pool) -------------------------------------
AMAX_MAX_BLOCKS = 16384   # kernels.h: a launch that keeps a magnitude record may have at most this many blocks


def pool_plan(C, H, W, M, pad):
    """conv.hip conv_igemm's "fused max pool" rule for a 3x3 launch that is offered an IgemmPool and stores plainly: the
    launch takes the pool when the fixed 4 x 32 tile (64-row M tiles) leaves ONE K split (the first-layer instantiation,
    Cin <= 4, never splits) and costs no more rounds of 256 blocks than the tile of choose_tile would."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    assert Ho > 0 and Wo > 0
    free = igemm_plan(C, H, W, M, 3, pad)
    mTiles = conv_mpad(M) // 64
    nChunks = cdiv(C, conv_cc(3))
    slots, minChunks = 256 * IG_BPC, max(1, cdiv(200, conv_cc(3) * 9))

    def splits_for(blocks):
        return min(min(max(1, slots // blocks), IG_MAX_SPLITS), max(1, nChunks // minChunks))

    blocks = cdiv(Wo, 32) * cdiv(Ho, 4) * mTiles
    first = C <= 4
    one_split = first or splits_for(blocks) == 1
    tile_refused = cdiv(blocks, 256) > cdiv(free["blocks"], 256)
    fused = one_split and not tile_refused
    return dict(C=C, M=M, Ho=Ho, Wo=Wo, Hp=(Ho - 1) // 2 + 1, Wp=(Wo - 1) // 2 + 1, first=first, mTiles=mTiles, blocks=blocks,
                free_blocks=free["blocks"], one_split=one_split, tile_refused=tile_refused, fused=fused,
                splits_wanted=1 if first else splits_for(blocks), could_split=(not first) and nChunks // minChunks > 1,
                tilesX=cdiv(Wo, 32), tilesY=cdiv(Ho, 4), lastChunkChannels=C - (cdiv(C, 4 if first else 8) - 1) * (4 if first else 8),
                cc=4 if first else 8,
                # the launch that runs: the fixed tile in one split, or conv_igemm's free plan with the pooling kernel behind it
                K=C * 9, splitK=1 if fused else free["splitK"], grid=blocks if fused else free["blocks"] * free["splitK"],
                late_record=fused and blocks > AMAX_MAX_BLOCKS)


def pool_labels(p):
    L = {"first_kernel" if p["first"] else "generic_kernel"}
    if p["fused"]:
        L.add("fused")
        L.add("fused_first" if p["first"] else "fused_generic")
        if p["mTiles"] > 1:
            L.add("m_tiles")
        if p["M"] % 64:
            L.add("rows_beyond_m")
        if p["M"] == 1:
            L.add("m1")
        if p["Wo"] < 32:
            L.add("wo_below_32")
        if p["Ho"] == 1 and p["Wo"] == 1:
            L.add("one_pixel")
        else:
            if p["Wo"] == 1:
                L.add("wo1")
            if p["Ho"] == 1:
                L.add("ho1")
        if p["Ho"] % 2 and p["Ho"] > 1:
            L.add("odd_ho")
        if p["Wo"] % 2 and p["Wo"] > 1:
            L.add("odd_wo")
        if p["tilesX"] > 1 and p["Wo"] % 32:
            L.add("ragged_x")
        if p["tilesY"] > 1 and p["Ho"] % 4:
            L.add("ragged_y")
        if p["lastChunkChannels"] < p["cc"]:
            L.add("last_chunk_partial")
        if p["could_split"]:
            L.add("one_split_by_full_grid")
        L.add("late_record" if p["late_record"] else "record_in_launch")
    else:
        L.add("not_fused")
        if not p["one_split"]:
            L.add("refused_by_splits")
        if p["tile_refused"]:
            L.add("refused_by_tile_first" if p["first"] else "refused_by_tile_generic")
    return L


POOL_CASES = [
    case("p_first_odd", (3, 5, 7, 64), "fused_first", "odd_ho", "odd_wo", "wo_below_32", "record_in_launch"),
    case("p_first_m20", (3, 5, 7, 20), "fused_first", "rows_beyond_m"),
    case("p_first_m1_wide", (3, 9, 67, 1), "fused_first", "m1", "ragged_x", "odd_wo", "ragged_y"),
    case("p_one_pixel", (1, 1, 1, 64), "fused_first", "one_pixel"),
    case("p_wo1", (3, 4, 1, 8), "fused_first", "wo1"),
    case("p_ho1", (3, 1, 40, 8), "fused_first", "ho1", "ragged_x"),
    case("p_generic_c9", (9, 13, 18, 20), "fused_generic", "last_chunk_partial", "rows_beyond_m", "odd_ho"),
    case("p_generic_m70", (40, 13, 18, 70), "fused_generic", "m_tiles", "rows_beyond_m"),
    case("p_generic_m130", (8, 6, 34, 130), "fused_generic", "m_tiles", "ragged_x"),
    case("p_generic_model", (16, 29, 50, 40), "fused_generic", "odd_ho", "ragged_x", "ragged_y"),
    case("p_full_grid", (48, 120, 700, 48), "fused_generic", "one_split_by_full_grid"),
    case("p_two_splits", (48, 13, 18, 48), "not_fused", "refused_by_splits", "generic_kernel"),
    case("p_four_splits", (96, 67, 91, 96), "not_fused", "refused_by_splits"),
    case("p_tile_first", (3, 65, 97, 130), "not_fused", "refused_by_tile_first"),
    case("p_tile_generic", (8, 65, 97, 130), "not_fused", "refused_by_tile_generic"),
    case("p_late_record", (1, 1026, 2046, 1), "fused_first", "late_record"),
]
POOL_PAD = 1
# what the issue's table says of those shapes: name -> (fused, blocks of the fixed tile, K splits of the launch that runs)
POOL_WANT = {
    "p_first_odd": (True, 2, 1), "p_first_m20": (True, 2, 1), "p_first_m1_wide": (True, 9, 1), "p_one_pixel": (True, 1, 1),
    "p_wo1": (True, 1, 1), "p_ho1": (True, 2, 1), "p_generic_c9": (True, 4, 1), "p_generic_m70": (True, 8, 1),
    "p_generic_m130": (True, 16, 1), "p_generic_model": (True, 16, 1), "p_full_grid": (True, 660, 1),
    "p_two_splits": (False, 4, 2), "p_four_splits": (False, 102, 4), "p_tile_first": (False, 272, 1),
    "p_tile_generic": (False, 272, 1), "p_late_record": (True, 16448, 1),
}
# variants of one fused case per kernel.  A variant names what differs from the base call (pool slope 0.25, no pool scale,
# a bias, a record, no input activation); "scale": entries of {0, 1} and one other (0.6; 0.75 in the exact-data run) -- a
# zero entry makes every window of its channel a four-way tie
POOL_VARIANT_BASES = ("p_first_m20", "p_generic_m70")
POOL_VARIANTS = ("scale", "slope_0", "slope_-0.5", "slope_1.5", "no_slope", "scale_no_slope", "in_act", "no_bias", "no_rec")
POOL_REQUIRED = {
    "first_kernel", "generic_kernel", "fused_first", "fused_generic", "not_fused", "refused_by_splits", "refused_by_tile_first",
    "refused_by_tile_generic", "m_tiles", "rows_beyond_m", "m1", "wo_below_32", "one_pixel", "wo1", "ho1", "odd_ho", "odd_wo",
    "ragged_x", "ragged_y", "last_chunk_partial", "one_split_by_full_grid", "late_record", "record_in_launch",
}


def pool_variant(name):
    """-> dict(slope, scale, in_act, bias, rec) of a POOL_VARIANTS name (None: the base call)"""
    v = dict(slope=0.25, scale=False, in_act=False, bias=True, rec=True)
    if name is None:
        return v
    assert name in POOL_VARIANTS, name
    if name.startswith("slope_"):
        v["slope"] = float(name[6:])
    elif name == "no_slope":
        v["slope"] = None
    elif name == "scale":
        v["scale"] = True
    elif name == "scale_no_slope":
        v["scale"], v["slope"] = True, None
    elif name == "in_act":
        v["in_act"] = True
    elif name == "no_bias":
        v["bias"] = False
    elif name == "no_rec":
        v["rec"] = False
    return v


# ---- conv.hip: weight gradient ----------------------------------------------------------------------------------------
WG_NT = 64          # gradient pixels per tile
WG_PM = 3           # patch slots per lane
W1_TH, W1_TW = 4, 64
W1_MAX_SLABS = 512
W1_TALL = 128       # wgrad_reduce_first: the tall fold from this many slabs


def choose_wgrad_tile(Ho, Wo, k, tys):
    best, bth, btw = -1, 2, 1
    for th in range(2, 9, 2):
        for tw in range(1, min(Wo, WG_NT // th) + 1):
            if tw < 8 and Wo >= 8:
                continue
            if (th + tys - 1) * (tw + k - 1) > 64 * WG_PM:
                continue
            tiles = cdiv(Ho, th) * cdiv(Wo, tw)
            cost = tiles * th * tw * (k * tys) + tiles * 64
            if best < 0 or cost < best or (cost == best and tw > btw):
                best, bth, btw = cost, th, tw
    return bth, btw


def wgrad_first_ok(Cin, O, k, Wo, act=False):
    """the first-layer kernel has no activating loader: a call with a slope or a scale takes the generic kernel"""
    return (not act) and k == 3 and Cin * 9 <= 32 and O <= 64 and Wo >= 2


def wgrad_plan(Cin, H, W, O, k, pad, act=False):
    """conv.hip wgrad_plan + launch_wgrad + wgrad_reduce_first"""
    assert k in (1, 3, 5, 7)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    assert Ho > 0 and Wo > 0
    if wgrad_first_ok(Cin, O, k, Wo, act):
        tilesX, tilesY = cdiv(Wo, W1_TW), cdiv(Ho, W1_TH)
        nSplit = min(W1_MAX_SLABS, tilesX * tilesY)
        return dict(kernel="first", k=k, Cin=Cin, O=O, Ho=Ho, Wo=Wo, TH=W1_TH, TW=W1_TW, tilesX=tilesX, tilesY=tilesY,
                    oTiles=1, cTiles=1, kyGroups=1, nSplit=nSplit, tilesPerBlock=cdiv(tilesX * tilesY, nSplit), PM=None,
                    pplane=None, tys=None, fold="tall" if nSplit >= W1_TALL else "plain", K=Ho * Wo, act=act,
                    slab_floats=nSplit * k * k * O * Cin)
    tys = 3 if k == 3 else 1
    TH, TW = choose_wgrad_tile(Ho, Wo, k, tys)
    tilesX, tilesY = cdiv(Wo, TW), cdiv(Ho, TH)
    oTiles, cTiles, kyGroups = cdiv(O, 64), cdiv(Cin, 64), k // tys
    base = oTiles * cTiles * kyGroups
    npix = tilesX * tilesY
    nSplit = max(1, min(npix, (512 + base // 2) // base))
    pplane = (TH + tys - 1) * (TW + k - 1)
    return dict(kernel="generic", k=k, Cin=Cin, O=O, Ho=Ho, Wo=Wo, TH=TH, TW=TW, tilesX=tilesX, tilesY=tilesY, oTiles=oTiles,
                cTiles=cTiles, kyGroups=kyGroups, nSplit=nSplit, tilesPerBlock=cdiv(npix, nSplit), PM=2 if pplane <= 128 else 3,
                pplane=pplane, tys=tys, fold="plain", K=Ho * Wo, act=act, slab_floats=nSplit * k * k * O * Cin)


def weight_gradient_plan(shape, act=False):
    C, H, W, O, k, pad = shape
    return wgrad_plan(C, H, W, O, k, pad, act)


def wgrad_workspace_floats(shape):
    """what conv_wgrad_workspace_bytes must cover for a conv.hip shape: either plan of it (the caller sizes the workspace
    before it knows whether the call carries an activation)"""
    return max(weight_gradient_plan(shape, False)["slab_floats"], weight_gradient_plan(shape, True)["slab_floats"])


def wgrad_labels(p):
    L = {"k%d" % p["k"], p["kernel"], "fold_" + p["fold"]}
    if p["act"]:
        L.add("act")
    if p["kernel"] == "first":
        tiles = p["tilesX"] * p["tilesY"]
        L.add("first_one_tile" if tiles == 1 else "first_plain_fold" if p["nSplit"] < W1_TALL else "first_tall_fold")
        if tiles > W1_MAX_SLABS:
            L.add("first_slab_cap")
    else:
        L.add("pm%d" % p["PM"])
        L.add("one_pixel_tile" if p["nSplit"] == 1 else "many_pixel_tiles")
        if p["tilesPerBlock"] > 1:
            L.add("block_walks_tiles")
        if p["O"] % 64:
            L.add("ragged_o")
        if p["Cin"] % 64:
            L.add("ragged_c")
        if p["oTiles"] > 1:
            L.add("o_tiles")
        if p["cTiles"] > 1:
            L.add("c_tiles")
        if p["k"] == 3 and p["Cin"] * 9 <= 36 and p["O"] <= 65:
            L.add("first_neighbour")
    return L


# ---- which operator-level calls reach conv.hip with the default options (split_bf16 = 1) ---------------------------------
def takes_split_form(role, shape, act=False):
    """api.cpp frcnn_conv2d_forward / _backward_input / _backward_weight with option split_bf16 on"""
    C, H, W, O, k, pad = shape
    if role == "forward":
        return WP.conv_x3_eligible(C, O, k) and (k == 3 or not act)
    if role == "input_gradient":
        return WP.conv_x3_eligible(O, C, k)
    assert role == "weight_gradient"
    return WP.conv_wgradx_eligible(C, O, k)


# tests/test_gpu_conv.py CASES (kept in step by tests/test_conv_plan.py)
GPU_CONV_CASES = [
    (3, 37, 53, 64, 3, 1), (16, 29, 50, 40, 3, 1), (64, 57, 100, 128, 3, 1), (24, 19, 23, 18, 1, 0), (20, 29, 50, 32, 3, 0),
    (10, 29, 50, 24, 5, 0), (6, 29, 50, 24, 7, 0), (130, 15, 17, 130, 3, 1), (256, 38, 63, 512, 3, 1), (512, 38, 63, 512, 3, 1),
    (512, 38, 63, 256, 7, 0),
]


# ---- case tables ------------------------------------------------------------------------------------------------------
def _m_sweep():
    out = []
    maps = {1: (33, 9, 11, 0), 3: (9, 9, 11, 1), 5: (5, 12, 14, 0), 7: (3, 13, 16, 0)}   # k -> (C, H, W, pad)
    for k, (C, H, W, pad) in maps.items():
        for M in (1, 18, 63, 64, 65, 128, 129):
            want = ["k%d" % k, "mpad%d" % min(conv_mpad(M), 256), "one_slab"]
            if k == 1:
                want.append("bm64" if M <= 64 else "bm128")
            else:
                want.append("bm64")
            if M == 1:
                want.append("m_below_18")
            out.append(case("m%d_k%d" % (M, k), (C, H, W, M, k, pad), *want))
    return out


IGEMM_CASES = _m_sweep() + [
    # channel counts around the chunk
    case("c1_k3", (1, 13, 18, 20, 3, 1), "first_layer", "last_chunk_partial"),
    case("c3_k3", (3, 13, 18, 20, 3, 1), "first_layer", "last_chunk_partial"),
    case("c4_k3", (4, 13, 18, 20, 3, 1), "first_layer"),
    case("c5_k3", (5, 13, 18, 20, 3, 1), "k3", "last_chunk_partial", "loader_dma"),
    case("c9_k3", (9, 13, 18, 20, 3, 1), "k3", "last_chunk_partial"),
    case("c31_k1", (31, 13, 18, 20, 1, 0), "k1", "last_chunk_partial", "loader_plain"),
    case("c33_k1", (33, 13, 18, 20, 1, 0), "k1", "last_chunk_partial"),
    case("c130_k1", (130, 13, 18, 20, 1, 0), "k1", "last_chunk_partial"),
    case("c5_k5", (5, 13, 18, 20, 5, 0), "k5", "zero_half_pair", "one_slab"),
    case("c13_k5", (13, 13, 18, 20, 5, 2), "k5", "zero_half_pair"),
    case("c17_k5", (17, 13, 18, 20, 5, 0), "k5", "zero_half_pair"),
    case("c5_k7", (5, 13, 18, 20, 7, 0), "k7", "zero_half_pair", "one_slab"),
    case("c13_k7", (13, 13, 18, 20, 7, 3), "k7", "zero_half_pair"),
    case("c17_k7", (17, 13, 18, 20, 7, 0), "k7", "zero_half_pair"),
    # maps: one output pixel
    case("pixel_k1", (33, 1, 1, 20, 1, 0), "k1", "one_pixel", "tw_below_8"),
    case("pixel_k3", (9, 3, 3, 20, 3, 0), "k3", "one_pixel"),
    case("pixel_k5", (5, 5, 5, 20, 5, 0), "k5", "one_pixel"),
    case("pixel_k7", (5, 7, 7, 20, 7, 0), "k7", "one_pixel"),
    # one output row of 128: the widest tile (on 5x5 and 7x7 the four-pass patch plane)
    case("row_k1", (33, 1, 128, 20, 1, 0), "k1", "one_row", "nit1"),
    case("row_k3", (9, 3, 130, 20, 3, 0), "k3", "one_row", "nit2"),
    case("row_k5", (5, 5, 132, 20, 5, 0), "k5", "one_row", "nit4"),
    case("row_k7", (5, 7, 134, 20, 7, 0), "k7", "one_row", "nit4"),
    # three output columns, forty rows: tiles narrower than 8
    case("narrow_k1", (33, 40, 3, 20, 1, 0), "k1", "tw_below_8"),
    case("narrow_k3", (9, 40, 3, 20, 3, 1), "k3", "tw_below_8"),
    case("narrow_k5", (5, 44, 7, 20, 5, 0), "k5", "tw_below_8", "nit2"),
    case("narrow_k7", (5, 46, 9, 20, 7, 0), "k7", "tw_below_8", "nit2"),
    # several tiles, the last one ragged in both directions
    case("ragged_k1", (33, 19, 21, 20, 1, 0), "k1", "ragged_x", "ragged_y", "many_blocks"),
    case("ragged_k3", (9, 19, 20, 70, 3, 1), "k3", "ragged_x", "ragged_y", "many_blocks", "nit1"),
    case("ragged_k5", (5, 23, 24, 20, 5, 0), "k5", "ragged_x", "ragged_y", "nit1"),
    case("ragged_k7", (5, 25, 26, 20, 7, 0), "k7", "ragged_x", "ragged_y", "nit2"),
    case("small_k7", (5, 11, 15, 20, 7, 0), "k7", "nit1"),
]

# split K on a map of one tile (9x11 outputs)
SPLITK_CASES = [
    case("split3_k3", (72, 9, 11, 20, 3, 1), "k3", "splitk", "splits_even"),
    case("split442_k3", (80, 9, 11, 20, 3, 1), "k3", "splitk", "last_split_short"),
    case("split_tail1_k3", (200, 9, 11, 20, 3, 1), "k3", "splitk", "last_split_one_chunk"),
    case("split24_k3", (576, 9, 11, 20, 3, 1), "k3", "splitk", "splitk_cap"),
    case("split_k1", (130, 9, 11, 20, 1, 0), "k1", "splitk", "last_chunk_partial", "bm64"),
    case("split_k1_bm128", (130, 9, 11, 70, 1, 0), "k1", "splitk", "last_chunk_partial", "bm128"),
    case("split_k5", (17, 13, 15, 20, 5, 0), "k5", "splitk", "zero_half_pair"),
    case("split_k7", (13, 15, 17, 20, 7, 0), "k7", "splitk", "zero_half_pair"),
]
# what the splits of those cases look like: name -> (splitK, chunksPerSplit, lastSplitChunks, lastChunkChannels)
SPLITK_WANT = {
    "split3_k3": (3, 3, 3, 8), "split442_k3": (3, 4, 2, 8), "split_tail1_k3": (7, 4, 1, 8), "split24_k3": (24, 3, 3, 8),
    "split_k1": (2, 3, 2, 2), "split_k1_bm128": (2, 3, 2, 2), "split_k5": (2, 5, 4, 1), "split_k7": (2, 4, 3, 1),
}

# fused input activation on the forward: (case name of a split-K shape, of a one-slab shape) per k
ACT_SHAPES = {
    1: ("split_k1", "c33_k1"), 3: ("split442_k3", "c9_k3"), 5: ("split_k5", "c5_k5"), 7: ("split_k7", "c5_k7"),
}
ACT_MODES = ("slope", "scale", "both")
ACT_EXTRA = [("c3_k3", "both"), ("split_k1_bm128", "both")]   # the first-layer instantiation; the 128-row 1x1 kernel
ACT_SCALE_TWO = ("c9_k3", "split_k5")                           # one scale entry of 2.0

IGEMM_REQUIRED = {
    "k1", "k3", "k5", "k7", "nit1", "nit2", "nit4", "bm64", "bm128", "mpad64", "mpad128", "mpad256", "first_layer",
    "loader_dma", "loader_plain", "splitk", "one_slab", "splitk_cap", "splits_even", "last_split_short",
    "last_split_one_chunk", "last_chunk_partial", "zero_half_pair", "m_below_18", "one_pixel", "one_row", "tw_below_8",
    "ragged_x", "ragged_y", "many_blocks",
}

WGRAD_CASES = [
    # the first-layer kernel
    case("first_c1_o1_tile", (1, 4, 30, 1, 3, 1), "first", "first_one_tile", "fold_plain"),
    case("first_c2_o17", (2, 9, 70, 17, 3, 1), "first", "first_plain_fold", "fold_plain"),
    case("first_c3_o64", (3, 37, 53, 64, 3, 1), "first", "first_plain_fold"),
    case("first_c3_o64_valid", (3, 14, 131, 64, 3, 0), "first", "first_plain_fold"),
    case("first_127", (3, 508, 20, 4, 3, 1), "first", "first_plain_fold"),
    case("first_128", (3, 512, 20, 4, 3, 1), "first", "first_tall_fold", "fold_tall"),
    case("first_tall_o17", (2, 64, 513, 17, 3, 1), "first", "first_tall_fold", "fold_tall"),
    case("first_cap", (3, 690, 190, 4, 3, 1), "first", "first_tall_fold", "first_slab_cap"),
    # ... and its neighbours on the generic kernel
    case("near_first_wo1", (3, 20, 3, 64, 3, 0), "generic", "first_neighbour"),
    case("near_first_o65", (3, 20, 30, 65, 3, 1), "generic", "first_neighbour", "o_tiles"),
    case("near_first_c4", (4, 20, 30, 64, 3, 1), "generic", "first_neighbour"),
    # the generic kernel: ragged 64-tiles of filters and channels
    case("k3_o1_c130", (130, 20, 30, 1, 3, 1), "generic", "k3", "ragged_o", "ragged_c", "c_tiles", "many_pixel_tiles"),
    case("k3_o130_c1", (1, 20, 30, 130, 3, 1), "generic", "k3", "ragged_o", "ragged_c", "o_tiles"),
    case("k3_o63_c65", (65, 20, 30, 63, 3, 1), "generic", "k3", "ragged_o", "ragged_c"),
    case("k3_o65_c63", (63, 8, 8, 65, 3, 1), "generic", "k3", "one_pixel_tile", "pm2"),
    case("k3_wide_tile", (20, 2, 32, 24, 3, 1), "generic", "k3", "one_pixel_tile", "pm3"),
    case("k3_wide_tiles", (20, 10, 128, 24, 3, 1), "generic", "k3", "many_pixel_tiles", "pm3"),
    case("k3_walk", (130, 40, 100, 130, 3, 1), "generic", "k3", "block_walks_tiles", "o_tiles", "c_tiles"),
    case("k1_o1_c130", (130, 20, 30, 1, 1, 0), "generic", "k1", "ragged_o", "c_tiles", "many_pixel_tiles"),
    case("k1_o130_c63", (63, 20, 30, 130, 1, 0), "generic", "k1", "ragged_c", "o_tiles"),
    case("k1_o65_c65_tile", (65, 8, 8, 65, 1, 0), "generic", "k1", "one_pixel_tile"),
    case("k5_o1_c65", (65, 20, 30, 1, 5, 0), "generic", "k5", "ragged_o", "c_tiles", "many_pixel_tiles"),
    case("k5_o130_c1", (1, 20, 30, 130, 5, 2), "generic", "k5", "ragged_c", "o_tiles"),
    case("k5_o63_c63_tile", (63, 12, 12, 63, 5, 0), "generic", "k5", "one_pixel_tile"),
    case("k7_o1_c63", (63, 20, 30, 1, 7, 0), "generic", "k7", "ragged_o", "ragged_c", "many_pixel_tiles"),
    case("k7_o65_c1", (1, 20, 30, 65, 7, 3), "generic", "k7", "ragged_c", "o_tiles"),
    case("k7_o130_c65_tile", (65, 14, 14, 130, 7, 0), "generic", "k7", "one_pixel_tile", "o_tiles", "c_tiles"),
    case("k7_walk", (130, 30, 40, 130, 7, 0), "generic", "k7", "block_walks_tiles"),
]
# fused input activation of the weight gradient: generic shapes of each k, and the first-layer shape (which then has to
# take the generic kernel)
WGRAD_ACT_CASES = ["k1_o130_c63", "k3_o63_c65", "k3_wide_tiles", "k5_o1_c65", "k7_o65_c1", "first_c3_o64", "first_c2_o17"]

WGRAD_REQUIRED = {
    "k1", "k3", "k5", "k7", "first", "generic", "fold_plain", "fold_tall", "first_one_tile", "first_plain_fold",
    "first_tall_fold", "first_slab_cap", "first_neighbour", "pm2", "pm3", "one_pixel_tile", "many_pixel_tiles",
    "block_walks_tiles", "ragged_o", "ragged_c", "o_tiles", "c_tiles",
}

# ---- conv.hip: the first layer's weight gradient from the pooled map's gradient (frcnn_conv2d_backward_weight_pooled) ------
def first_pooled_eligible(C, O, Wo):
    """conv_wgrad_first_pooled_eligible (k = 3): one MFMA column must stay free for the column of ones, hence < 32"""
    return C * 9 < 32 and O <= 64 and Wo >= 2


def first_pooled_plan(C, H, W, O, pad):
    """conv.hip conv_wgrad_first_pooled: conv_wgrad_first_kernel<3, true> on 4 x 64 tiles, one slab slice per block, O + 1
    floats (bias sums, slope sum) behind every slice.  wgrad_reduce_first takes the tall fold whenever there are extras, so
    the 127 / 128 slab boundary of the un-fused kernel is no boundary of the fold here: the cases on either side of it stay
    (they mirror the first_* cases of WGRAD_CASES), and the label says which side they are on."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    assert Ho > 0 and Wo > 0 and first_pooled_eligible(C, O, Wo)
    tilesX, tilesY = cdiv(Wo, W1_TW), cdiv(Ho, W1_TH)
    tiles = tilesX * tilesY
    nSplit = min(W1_MAX_SLABS, tiles)
    return dict(Cin=C, O=O, Ho=Ho, Wo=Wo, Hp=(Ho - 1) // 2 + 1, Wp=(Wo - 1) // 2 + 1, tilesX=tilesX, tilesY=tilesY, tiles=tiles,
                nSplit=nSplit, tilesPerBlock=cdiv(tiles, nSplit), fold="tall", ones_lane=9 * C, K=Ho * Wo,
                slab_floats=nSplit * (9 * O * C + O + 1))


# The slope gradient's summation order, from conv_wgrad_first_kernel<3, true>: a thread owns one 2x2 window of a tile and the
# 16 channels of its wave, and chains its 4 * 16 = 64 terms x * g of that tile -- and of every further tile its block walks --
# with one fmaf each (one rounding per term; the product is not rounded); then 6 xor-shuffle levels inside the wave and 2
# levels over the four waves, (r0 + r1) + (r2 + r3).  A term therefore passes at most 64 * tilesPerBlock + 6 + 2 roundings
# before it leaves the block.  The fold of the nSplit block sums and the accumulating store are rounding_bound's S and + 2.
W1_SLOPE_CHAIN = 64     # terms per lane chain and tile
W1_SLOPE_LEVELS = 6 + 2  # shuffle levels of a 64-lane wave, levels over four waves


def first_pooled_slope_terms(p):
    return W1_SLOPE_CHAIN * p["tilesPerBlock"] + W1_SLOPE_LEVELS


def first_pooled_labels(p):
    L = {"ones_lane_%d" % p["ones_lane"]}
    L.add("one_tile" if p["tiles"] == 1 else "slabs_below_128" if p["nSplit"] < W1_TALL else "slabs_from_128")
    if p["tiles"] > W1_MAX_SLABS:
        L.add("block_walks_tiles")
    if p["tiles"] % p["nSplit"] or p["tilesPerBlock"] == 1:
        L.add("prefetch_past_the_end")   # a block whose next tile does not exist issues that tile's loads all the same
    if p["O"] % 16:
        L.add("o_not_multiple_of_16")
    if p["O"] < 16:
        L.add("idle_waves")
    if p["Wo"] % 2:
        L.add("shifted_column")
        if p["Wo"] % W1_TW == 1:
            L.add("shifted_opens_tile")
    if p["Wo"] == 2:
        L.add("wo2")
    if p["Wo"] % W1_TW and p["tilesX"] > 1:
        L.add("ragged_x")
    if p["Ho"] == 1:
        L.add("ho1")
    elif p["Ho"] % 2:
        L.add("odd_ho")
    if p["Ho"] % W1_TH:
        L.add("ragged_y")
    return L


# (C, H, W, O, pad); the first eight mirror the first_* cases of WGRAD_CASES
FIRST_POOLED_CASES = [
    case("fp_c1_o1_tile", (1, 4, 30, 1, 1), "one_tile", "ones_lane_9", "idle_waves"),
    case("fp_c2_o17", (2, 9, 70, 17, 1), "ones_lane_18", "o_not_multiple_of_16", "slabs_below_128", "ragged_x", "odd_ho"),
    case("fp_c3_o64", (3, 37, 53, 64, 1), "ones_lane_27", "shifted_column", "odd_ho"),
    case("fp_c3_o64_valid", (3, 14, 131, 64, 0), "shifted_opens_tile", "ragged_x"),
    case("fp_wo2", (3, 3, 2, 5, 1), "wo2", "one_tile", "o_not_multiple_of_16", "idle_waves"),
    case("fp_ho1", (3, 1, 4, 8, 1), "ho1", "one_tile"),
    case("fp_127", (3, 508, 20, 4, 1), "slabs_below_128"),
    case("fp_128", (3, 512, 20, 4, 1), "slabs_from_128"),
    case("fp_tall_o17", (2, 64, 513, 17, 1), "slabs_from_128", "shifted_opens_tile", "o_not_multiple_of_16"),
    case("fp_cap", (3, 690, 190, 4, 1), "block_walks_tiles", "prefetch_past_the_end"),
]
FIRST_POOLED_MIRROR = {   # name -> the un-fused case of WGRAD_CASES with the same shape
    "fp_c1_o1_tile": "first_c1_o1_tile", "fp_c2_o17": "first_c2_o17", "fp_c3_o64": "first_c3_o64",
    "fp_c3_o64_valid": "first_c3_o64_valid", "fp_127": "first_127", "fp_128": "first_128", "fp_tall_o17": "first_tall_o17",
    "fp_cap": "first_cap",
}
# shapes the entry point must refuse: name -> ((C, H, W, O, pad), slope given)
FIRST_POOLED_ERRORS = {
    "c4": ((4, 8, 8, 8, 1), True), "o65": ((3, 8, 8, 65, 1), True), "wo1": ((3, 8, 1, 8, 1), True),
    "no_slope": ((3, 8, 8, 8, 1), False),
}
FIRST_POOLED_REQUIRED = {
    "ones_lane_9", "ones_lane_18", "ones_lane_27", "one_tile", "slabs_below_128", "slabs_from_128", "block_walks_tiles",
    "prefetch_past_the_end", "o_not_multiple_of_16", "idle_waves", "shifted_column", "shifted_opens_tile", "wo2", "ragged_x",
    "ho1", "odd_ho", "ragged_y",
}


def find_pool(name):
    for c in POOL_CASES + FIRST_POOLED_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


# call-order independence: (role, case A, activation of A, role, case B, activation of B)
ORDER_PAIRS = [
    ("forward", "split24_k3", None, "forward", "split_tail1_k3", None),
    ("forward", "split_k1", None, "forward", "ragged_k1", None),
    ("forward", "split_k7", "both", "forward", "split_k5", None),
    ("input_gradient", "split442_k3", None, "forward", "split24_k3", None),
    ("weight_gradient", "k3_walk", None, "weight_gradient", "k7_walk", None),
    ("weight_gradient", "first_tall_o17", None, "weight_gradient", "first_128", None),
    ("weight_gradient", "first_c3_o64", None, "weight_gradient", "first_c3_o64", "slope"),
    ("weight_gradient", "first_c3_o64", "slope", "weight_gradient", "first_c3_o64", None),
]


def find(name):
    for c in IGEMM_CASES + SPLITK_CASES + WGRAD_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


# ---- fp64 references and the rounding bound ---------------------------------------------------------------------------
U = 2.0 ** -24   # unit roundoff of fp32


def activate(x, slope, scale):
    """the loaders' fused activation, in fp32 as they compute it: PReLU with one slope, then the channel's dropout scale"""
    x = np.asarray(x, np.float32)
    if slope is not None:
        x = np.where(x > 0, x, np.float32(slope) * x).astype(np.float32)
    if scale is not None:
        x = (x * np.asarray(scale, np.float32)[:, None, None]).astype(np.float32)
    return x


def ref_forward(x, w, b, pad):
    """fp64 by the definition: out[o] = b[o] + sum_c sum_taps w[o][c][ky][kx] x[c][y + ky - pad][x + kx - pad]"""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    C, H, W = x.shape
    O, _, k, _ = w.shape
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((O, Ho * Wo))
    for ky in range(k):
        for kx in range(k):
            out += w[:, :, ky, kx] @ xp[:, ky:ky + Ho, kx:kx + Wo].reshape(C, -1)
    if b is not None:
        out += np.asarray(b, np.float64)[:, None]
    return out.reshape(O, Ho, Wo)


def ref_input_gradient(g, w, pad, H, W):
    w = np.asarray(w, np.float64)
    k = w.shape[2]
    wt = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    out = ref_forward(g, wt, None, k - 1 - pad)
    assert out.shape[1:] == (H, W)
    return out


def ref_weight_gradient(x, g, k, pad):
    x = np.asarray(x, np.float64); g = np.asarray(g, np.float64)
    C = x.shape[0]
    O, Ho, Wo = g.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    gw = np.zeros((O, C, k, k))
    g2 = g.reshape(O, -1)
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = g2 @ xp[:, ky:ky + Ho, kx:kx + Wo].reshape(C, -1).T
    return gw, g2.sum(1)


def rounding_bound(K, S, mag):
    """|fl(sum) - sum| <= (K + S + 2) u mag: K products rounded once each and added in any order in fp32 (K - 1 additions),
    S slabs folded (S - 1), a bias or an accumulating destination added (2 more), to first order in u; mag = the same sum
    over magnitudes"""
    return (K + S + 2) * U * np.asarray(mag, np.float64)


# ---- the pooling of the epilogue and its backward, restated -------------------------------------------------------------
POOL_WINDOW = ((0, 0), (0, 1), (1, 0), (1, 1))   # code dy * 2 + dx


def pool_act_fp32(x, slope, scale):
    """elem.hip maxpool_act_forward_kernel in numpy float32: act = PReLU, then the channel's scale (activate(): one rounding
    each, no fused multiply-add), then the 2x2 stride-2 ceil-mode window in the order (0,0), (0,1), (1,0), (1,1) with a strict
    `>`: the first maximum wins.  -> (pooled float32 [C][Hp][Wp], code uint8)"""
    a = activate(x, slope, scale)
    C, H, W = a.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = np.ascontiguousarray(a[:, 0::2, 0::2])
    assert best.shape == (C, Hp, Wp) and best.dtype == np.float32
    code = np.zeros((C, Hp, Wp), np.uint8)
    for e, (dy, dx) in enumerate(POOL_WINDOW[1:], 1):
        v = a[:, dy::2, dx::2]
        cand = np.full((C, Hp, Wp), -np.inf, np.float32)   # a position outside the map never wins
        cand[:, :v.shape[1], :v.shape[2]] = v
        take = cand > best
        best = np.where(take, cand, best)
        code[take] = e
    return best, code


def pool_route(gpool, code, Ho, Wo):
    """the pool's backward: every pooled gradient goes to the position its code names (which must lie inside the map)"""
    gpool = np.asarray(gpool, np.float64)
    C, Hp, Wp = gpool.shape
    out = np.zeros((C, 2 * Hp, 2 * Wp))
    for e, (dy, dx) in enumerate(POOL_WINDOW):
        out[:, dy::2, dx::2] = np.where(code == e, gpool, 0.0)
    assert not out[:, Ho:, :].any() and not out[:, :, Wo:].any(), "a code names a position outside the map"
    return np.ascontiguousarray(out[:, :Ho, :Wo])


def ref_pooled_weight_gradient(inp, gpool, code, x, slope, pad):
    """fp64 by the definition -> (gw, gb, gslope) and the same sums over magnitudes (mw, mb, mslope)"""
    x = np.asarray(x, np.float64)
    _, Ho, Wo = x.shape
    r = pool_route(gpool, code, Ho, Wo)
    g = r * np.where(x > 0, 1.0, float(slope))
    gw, gb = ref_weight_gradient(inp, g, 3, pad)
    mw, mb = ref_weight_gradient(np.abs(np.asarray(inp, np.float64)), np.abs(g), 3, pad)
    neg = x <= 0
    return (gw, gb, float((x * r)[neg].sum())), (mw, mb, float(np.abs(x * r)[neg].sum()))


def assert_exact_in_fp32(mag, quantum, what=""):
    """Every partial sum of a sum whose terms are multiples of `quantum` and whose magnitudes add up to `mag` is a multiple
    of `quantum` below `mag`: exactly representable in fp32, in whatever order the terms are added, when mag / quantum < 2^24"""
    top = float(np.max(mag)) / quantum
    assert top < 2.0 ** 24, "%s: sum of magnitudes %g quanta: the exact-data run would round" % (what, top)
