"""The tables of tests/test_gpu_widths.py reach every planner branch they exist for (tests/width_plan.py restates the
shape rules; no GPU needed).  A later edit of the tables cannot drop a branch without this failing."""
import width_plan as WP


def _positions(filters, heads, H, W):
    """Positions of every anchor net's output map: 'same' 3x3 convolutions, ceil-mode 2x2 pooling per block
    (model_utilities.lua:23), then the valid k x k head convolution (:31)."""
    maps, h, w = [], H, W
    for _ in filters:
        h, w = -(-(h - 2) // 2) + 1, -(-(w - 2) // 2) + 1
        maps.append((h, w))
    return [(maps[i - 1][0] - k + 1) * (maps[i - 1][1] - k + 1) for k, n, i in heads]


def test_tables_reach_every_branch():
    labels = set()
    for c in WP.CONFIGS.values():
        labels |= WP.labels_of_config(c)
    labels |= WP.labels_of_sweep()
    labels |= WP.labels_of_compact()
    assert WP.REQUIRED <= labels, sorted(WP.REQUIRED - labels)


def test_each_configuration_labels_what_its_comment_names():
    want = {
        "backbone_48_96_192_320": {"igemm_f32", "x3_forward_f32_input_gradient", "x3_bm64", "sparse_one_split", "compact_on"},
        "mixed_anchor_nets": {"x3_bm128", "x3_bm64", "sparse_several_splits"},
        "vgg_small_n128": {"sparse_several_splits", "cnet_split_on"},
        "cnet_1000_500": {"cnet_split_off"},
        "cnet_2304_512": {"cnet_split_on", "cnet_split_off"},
    }
    assert set(want) == set(WP.CONFIGS)
    for name, c in WP.CONFIGS.items():
        got = WP.labels_of_config(c)
        assert want[name] <= got, (name, sorted(want[name] - got))
    # the classification widths that are no multiples of 16 never take the split product, whatever R
    assert "cnet_split_on" not in WP.labels_of_config(WP.CONFIGS["cnet_1000_500"])
    # 96 -> 192: split forward, fp32 input gradient, in the same convolution
    assert [(c[2], c[3], c[4], c[5]) for c in WP.backbone_convs([48, 96, 192, 320]) if c[2] == 96 and c[3] == 192] == \
        [(96, 192, True, False)]


def test_positions_fit_the_maps():
    for c in list(WP.CONFIGS.values()) + list(WP.COMPACT_CONFIGS.values()):
        assert len(c["heads"]) == len(c["positions"]) == WP.SCALES
        assert all(0 < P <= m for P, m in zip(c["positions"], _positions(c["filters"], c["heads"], *c["frame"])))
        assert all(P > 0 for P in _positions(c["filters"], c["heads"], *WP.SMALL))
    for n in WP.SWEEP_WIDTHS:
        assert min(_positions(WP.VGG_BACKBONE, WP.vgg_heads(n), *WP.SWEEP_FRAME)) > max(WP.SWEEP_POSITIONS)
    # the 7x7 net of the bug configuration: 12 x 18 positions at 288 x 384, more than 70 of them sampled
    c = WP.CONFIGS["vgg_small_n128"]
    assert _positions(c["filters"], c["heads"], *c["frame"])[3] == 12 * 18 and c["positions"][3] > 70


def test_compact_boundaries_are_labelled():
    for c in WP.COMPACT_CONFIGS.values():
        for b, C in enumerate(c["filters"]):
            if WP.compact_plan(c["filters"], b, C) is None:
                continue
            assert WP.compact_plan(c["filters"], b, C - 16) == "compact"
            assert WP.compact_plan(c["filters"], b, C - 15) == "skipped"
            assert WP.compact_plan(c["filters"], b, C) == "skipped"
            assert WP.compact_plan(c["filters"], b, 1) == "compact"
    widths = {C for c in WP.COMPACT_CONFIGS.values() for b, C in enumerate(c["filters"])
              if WP.compact_plan(c["filters"], b, C - 16) == "compact"}
    assert {128, 192, 256, 320, 384} <= widths
    # 96 -> 192 has no split input gradient: that 192 block cannot run compact; behind a 128 block it can
    assert WP.compact_plan([48, 96, 192, 320], 2, 100) is None
    assert WP.compact_plan([64, 128, 192, 320], 2, 100) == "compact"


def test_head_splits_fit_the_slab():
    """heads_jobs: splits * P <= 4096 (the K-split slab) for every width, input and P <= 512; the cap changes nothing for
    n >= 256, where 256 / tiles already kept the product under the bound.  Before the cap, narrower nets overflowed from
    the position counts the sweep brackets (70 on the 7x7 net of vgg_small's block 4, 456 on the 3x3 net of block 3)."""
    for n in (24, 48, 64, 96, 128, 192, 256, 320, 384, 512):
        for cin in (16, 48, 96, 128, 192, 256, 320, 384, 512):
            for k in (3, 5, 7):
                for P in range(1, WP.SPARSE_MAX_POS + 1):
                    s = WP.head_splits(n, cin, k, P)
                    assert 1 <= s and s * P <= 4096, (n, cin, k, P, s)
                    if n >= 256:
                        assert s == WP.head_splits(n, cin, k, P, capped=False)

    def first_overflow(n, cin, k):
        return next((P for P in range(1, 513) if WP.head_splits(n, cin, k, P, capped=False) * P > 4096), None)
    for n in (64, 128):
        assert [first_overflow(n, 256, 3), first_overflow(n, 384, 3), first_overflow(n, 384, 5), first_overflow(n, 384, 7)] == \
            [456, 342, 121, 70]
    assert first_overflow(192, 384, 7) == 98
    assert {69, 70, 455, 456} <= set(WP.SWEEP_POSITIONS)
