"""The model tables of tests/test_gpu_widths.py and a plain restatement of the shape rules that decide which code path a
launch takes (csrc/convx.hip, csrc/wgradx.hip, csrc/gemmx.hip, csrc/net.cpp), with the library's default options.

The restatement only LABELS the GPU cases with the branches they reach, so that tests/test_width_plan.py can check
that the tables still reach every one of them: it is no evidence that a branch computes the right thing.  The GPU
tests against the oracle are."""

VGG_BACKBONE = [64, 128, 256, 384]
SCALES = 4   # cfg["scales"] has four entries: always four anchor nets


def cdiv(a, b):
    return -(-a // b)


def layers_of(filters):
    """A backbone in the form of models/vgg_small.lua: one convolution in the first block, two in every other, a
    SpatialDropout of 0.4 behind the first convolution of every block but the first."""
    return [dict(filters=f, kW=3, kH=3, padW=1, padH=1, dropout=0.0 if b == 0 else 0.4, conv_steps=1 if b == 0 else 2)
            for b, f in enumerate(filters)]


def heads_of(spec):
    """[(k, n, input block)] -> anchor_nets"""
    return [dict(kW=k, n=n, input=i) for k, n, i in spec]


def cls_of(n1, n2):
    return [dict(n=n1, dropout=0.5, batch_norm=True), dict(n=n2, dropout=0.5)]


def vgg_heads(n):
    """vgg_small's four anchor nets (3x3 on block 3, 3x3 / 5x5 / 7x7 on block 4), all n wide."""
    return [(3, n, 3), (3, n, 4), (5, n, 4), (7, n, 4)]


# ---- the shape rules --------------------------------------------------------------------------------------------------
SPARSE_MAX_POS = 512   # net.cpp SPARSE_MAX_POS: more sampled positions on one anchor net -> the dense convolutions


def conv_x3_eligible(Cin, M, k):
    """convx.hip conv_x3_eligible: the split-bf16 convolution (CX_CH = 16 channels per chunk)."""
    return k in (3, 5, 7) and Cin % 16 == 0 and Cin >= 16 and M % (64 if k == 3 else 128) == 0


def conv_x3_bm(M, k):
    """convx.hip conv_x3_bm, the M % 128 part: 64-filter blocks when 128 does not divide M, 128-filter blocks for a 5x5 /
    7x7 launch that it divides.  None: a 3x3 launch whose choice the tile count makes."""
    if M % 128:
        return 64
    return 128 if k != 3 else None


def conv_wgradx_eligible(Cin, O, k):
    """wgradx.hip conv_wgradx_eligible"""
    return k == 3 and Cin % 64 == 0 and O % 64 == 0


def conv_forms(Cin, Cout, k, backbone, need_dgrad):
    """net.cpp ensure_conv: (x_f, x_d) = the forward / input-gradient launches take the split form.  An anchor net's
    convolution (backbone=False) is split forward at any k; its input gradient is never split."""
    x_f = (k == 3 or not backbone) and conv_x3_eligible(Cin, Cout, k)
    x_d = backbone and need_dgrad and conv_x3_eligible(Cout, Cin, k)
    return x_f, x_d


def backbone_convs(filters):
    """[(block, step, Cin, Cout, x_f, x_d)] of a backbone in the form of layers_of (net.cpp ensure_shapes: the very first
    convolution computes no input gradient)."""
    out, cin = [], 3
    for b, l in enumerate(layers_of(filters)):
        for st in range(l["conv_steps"]):
            x_f, x_d = conv_forms(cin, l["filters"], 3, True, not (b == 0 and st == 0))
            out.append((b, st, cin, l["filters"], x_f, x_d))
            cin = l["filters"]
    return out


def compact_plan(filters, b, nk):
    """net.cpp plan_compact for block b with nk of its C filters kept: "compact" (the block leaves the dropped channels
    out), "skipped" (eligible, but nothing to leave out: nk == 0 or nkK = min(C, ceil16(nk)) >= C) or None (the block's
    convolutions do not take the fused split form at all)."""
    layers = layers_of(filters)
    l = layers[b]
    C = l["filters"]
    if l["dropout"] <= 0 or l["conv_steps"] < 2:
        return None
    convs = [c for c in backbone_convs(filters) if c[0] == b]
    (_, _, cin, _, f0, d0), (_, _, _, _, f1, d1) = convs[:2]
    if not (f0 and f1 and d1 and (b == 0 or d0)):
        return None
    nkM, nkK = min(C, cdiv(nk, 64) * 64), min(C, cdiv(nk, 16) * 16)
    if nk == 0 or nkK >= C:
        return "skipped"
    if (not conv_x3_eligible(cin, nkM, 3) or not conv_x3_eligible(nkK, C, 3) or not conv_x3_eligible(C, nkM, 3) or
            (b > 0 and not conv_x3_eligible(nkK, cin, 3)) or not conv_wgradx_eligible(nkM, C, 3) or
            not conv_wgradx_eligible(cin, nkM, 3)):
        return "skipped"
    return "compact"


def head_splits(n, Cin, k, P, capped=True):
    """heads.hip heads_plan_splits (net.cpp heads_jobs through heads_add_job): the K splits of the sparse anchor net's product HX = W COL^T at P positions.  capped=False: the
    rule before the cap at 4096 / P (the K-split slab holds n x 4096 partial sums)."""
    ckk = Cin * k * k
    tiles = cdiv(n, 64) * cdiv(P, 64)
    bounds = [ckk // 256, 64, 256 // tiles] + ([4096 // P] if capped else [])
    splits = max(1, min(bounds))
    per = cdiv(cdiv(ckk, splits), 32) * 32
    return cdiv(ckk, per)


def linear_x_eligible(role, R, I, O):
    """gemmx.hip linear_x_eligible (role 1 forward, 2 input gradient, 4 weight gradient)."""
    if I % 16 or O % 16 or R < 32 or R * I * O < 1.0e9:
        return False
    return role == 2 or R >= 192


# ---- the tables of tests/test_gpu_widths.py --------------------------------------------------------------------------
# part 1: model configurations, each checked against the oracle through pnet:forward/backward (the anchor nets as dense
# convolutions) on a small odd frame and through the whole objective (sparse anchor nets, compact blocks on) with
# `positions` distinct sampled positions per anchor net on frame `frame`.
SMALL = (133, 181)
CONFIGS = {
    # fp32 implicit GEMM at 48 / 96 filters, split forward with fp32 input gradient (96 -> 192), 64-filter split blocks (192,
    # 320), a compact 320 block; the first anchor net on the 48-filter block: ckk < 512, one K split
    "backbone_48_96_192_320": dict(filters=[48, 96, 192, 320], heads=[(3, 64, 1), (3, 64, 3), (5, 64, 4), (7, 64, 4)],
                                   cls=(256, 128), frame=SMALL, positions=(40, 24, 12, 6)),
    # one grouped launch of anchor nets that differ in width, ckk and form (dense: 3x3 128 / 192 split, 5x5 128 split with
    # 128-filter blocks, 7x7 64 fp32); hd_grid / heads_act_backward sized by the largest job
    "mixed_anchor_nets": dict(filters=VGG_BACKBONE, heads=[(3, 128, 3), (3, 192, 4), (5, 128, 4), (7, 64, 4)],
                              cls=(1024, 512), frame=SMALL, positions=(40, 30, 20, 10)),
    # the configuration of the heads_jobs K-split overflow: 128-wide anchor nets, more than 70 positions on the 7x7 net and
    # more than 120 on the 5x5 net (288 x 384: block 4 is 18 x 24, the 7x7 net has 12 x 18 positions)
    "vgg_small_n128": dict(filters=VGG_BACKBONE, heads=vgg_heads(128), cls=(1024, 512), frame=(288, 384),
                           positions=(20, 20, 130, 100)),
    # classification widths that are no multiples of 16: the large Linear never takes the split form
    "cnet_1000_500": dict(filters=VGG_BACKBONE, heads=vgg_heads(256), cls=(1000, 500), frame=SMALL,
                          positions=(40, 30, 20, 10)),
    # a classification net that takes the split form from R = 32 rows (input gradient) / 192 rows (every role)
    "cnet_2304_512": dict(filters=VGG_BACKBONE, heads=vgg_heads(256), cls=(2304, 512), frame=SMALL,
                          positions=(40, 30, 20, 10)),
}
# rows of the classification net's own forward / backward check, on either side of linear_x_eligible's R >= 32 / >= 192
CNET_CONFIGS = ("cnet_1000_500", "cnet_2304_512")
CNET_ROWS = (31, 32, 191, 192)
ROI_CELLS = 36   # 6 x 6 ROI pooling (config/duplo.lua)

# part 2: vgg_small's backbone at 450 x 800 (every anchor net has more than 513 positions), all four anchor nets n wide
# and P positions on each: the sparse anchor nets against the dense convolutions.  P = 513 is the fall-back to the dense
# convolutions inside the deferred pass.
SWEEP_FRAME = (450, 800)
SWEEP_WIDTHS = (64, 128, 192, 256, 320)
SWEEP_POSITIONS = (1, 64, 65, 69, 70, 455, 456, 512, 513)
# ... and one oracle-backed objective per width at vgg_small_n128's frame and positions (n = 128: that configuration itself)
ORACLE_WIDTHS = (64, 192, 256, 320)

# part 3: explicit keep vectors at the boundaries of plan_compact, kept count by block width C (every dropout block of
# the model at once), checked against the oracle
COMPACT_CONFIGS = {
    "backbone_64_128_192_320": dict(filters=[64, 128, 192, 320], heads=vgg_heads(64), cls=(256, 128), frame=SMALL,
                                    positions=(16, 12, 8, 4)),
    "vgg_small": dict(filters=VGG_BACKBONE, heads=vgg_heads(256), cls=(1024, 512), frame=SMALL, positions=(16, 12, 8, 4)),
}
COMPACT_KEPT = ("1", "63", "64", "65", "C-16", "C-15", "C")


def kept_count(spec, C):
    """"C-16" -> C - 16, "C" -> C, "64" -> 64"""
    if spec.startswith("C"):
        return C + int(spec[1:] or 0)
    return int(spec)


def random_kept(filters, seed=3):
    """Kept counts of the random keep vectors tests/test_gpu_model.py _masks draws for check_loss_and_gradient
    (RandomState(3), rand(C) > dropout, block by block)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    return [None if l["dropout"] <= 0 else int((rng.rand(l["filters"]) > l["dropout"]).sum()) for l in layers_of(filters)]


def examples(positions):
    """Examples of test_gpu_widths.py _examples for these positions: one per position, a second aspect at every fifth."""
    return sum(P + cdiv(P, 5) for P in positions)


# ---- labels -----------------------------------------------------------------------------------------------------------
def _conv_labels(filters, heads, labels):
    for b, st, cin, cout, x_f, x_d in backbone_convs(filters):
        if x_f:
            if conv_x3_bm(cout, 3):
                labels.add("x3_bm%d" % conv_x3_bm(cout, 3))
            if not (b == 0 and st == 0) and not x_d:
                labels.add("x3_forward_f32_input_gradient")
        elif cin >= 16:
            labels.add("igemm_f32")
    for k, n, i in heads:   # pnet:forward's anchor nets: the dense convolutions
        x_f, _ = conv_forms(filters[i - 1], n, k, False, True)
        if x_f and conv_x3_bm(n, k):
            labels.add("x3_bm%d" % conv_x3_bm(n, k))


def _head_labels(filters, heads, positions, labels):
    dense = any(P > SPARSE_MAX_POS for P in positions)
    for (k, n, i), P in zip(heads, positions):
        if P == SPARSE_MAX_POS:
            labels.add("P512")
        if P == SPARSE_MAX_POS + 1:
            labels.add("P513")
    if dense:
        labels.add("heads_dense_fallback")
        return
    for (k, n, i), P in zip(heads, positions):
        if P > 0:
            labels.add("sparse_one_split" if head_splits(n, filters[i - 1], k, P) == 1 else "sparse_several_splits")


def _cnet_labels(filters, cls, R, labels):
    I, O = ROI_CELLS * filters[-1], cls[0]
    roles = [r for r in (1, 2, 4) if linear_x_eligible(r, R, I, O)]
    labels.add("cnet_split_on" if roles else "cnet_split_off")


def labels_of_config(c):
    labels = set()
    _conv_labels(c["filters"], c["heads"], labels)
    _head_labels(c["filters"], c["heads"], c["positions"], labels)
    _cnet_labels(c["filters"], c["cls"], examples(c["positions"]), labels)
    for name in CNET_CONFIGS:
        if CONFIGS[name] is c:
            for R in CNET_ROWS:
                _cnet_labels(c["filters"], c["cls"], R, labels)
    for b, nk in enumerate(random_kept(c["filters"])):
        plan = nk is not None and compact_plan(c["filters"], b, nk)
        if plan:
            labels.add("compact_on" if plan == "compact" else "compact_skipped")
    return labels


def labels_of_sweep():
    labels = set()
    for n in SWEEP_WIDTHS:
        for P in SWEEP_POSITIONS:
            _head_labels(VGG_BACKBONE, vgg_heads(n), (P,) * SCALES, labels)
    return labels


def labels_of_compact():
    labels = set()
    for c in COMPACT_CONFIGS.values():
        for spec in COMPACT_KEPT:
            for b, C in enumerate(c["filters"]):
                plan = compact_plan(c["filters"], b, kept_count(spec, C))
                if plan:
                    labels.add("compact_on" if plan == "compact" else "compact_skipped")
    return labels


REQUIRED = {
    "x3_bm128", "x3_bm64", "x3_forward_f32_input_gradient", "igemm_f32", "sparse_one_split", "sparse_several_splits",
    "P512", "P513", "heads_dense_fallback", "compact_on", "compact_skipped", "cnet_split_on", "cnet_split_off",
}
