"""The tables of tests/test_gpu_cnet_shapes.py reach every branch of the classification net they exist for
(tests/cnet_plan.py restates the shape rules; no GPU needed).  A later edit of the tables cannot drop a branch without
this failing."""
import numpy as np

import cnet_plan as CP


def test_tables_reach_every_branch():
    labels = CP.labels_of_tables()
    assert CP.REQUIRED <= labels, sorted(CP.REQUIRED - labels)


# what each model is in the tables for: (table, L, class_count) -> labels it must reach
WANT = {
    ("std", 32, 16): {"fold_consumer+rows_keep", "fold_consumer+rows_tall", "fold_none+rows_keep", "fold_none+rows_tall",
                      "bn_fused", "heads_fused", "top_act_in_heads", "heads_grid_stride", "heads_partial_block"},
    ("std", 64, 16): {"fold_launch+rows_keep", "fold_launch+rows_tall"},
    ("ragged", 32, 16): {"ragged_width", "heads_unfused_nf"},
    ("bn_last", 32, 16): {"flat_fold", "top_bn", "bn_fold_consumer+rows_keep", "bn_fold_consumer+rows_tall"},
    ("bn_both", 32, 16): {"top_bn", "bn_fused"},
    ("wide_second", 32, 16): {"dgrad_fold_deferred", "top_act_in_heads"},
    ("one", 32, 16): {"one_layer", "top_bn"},
    ("three", 32, 16): {"three_layers", "top_bn"},
    ("none", 32, 16): {"no_hidden_layer", "heads_unfused_nf"},
    ("none", 16, 16): {"no_hidden_layer", "heads_on_input"},
    ("heads_1024", 32, 16): {"heads_lds_max", "heads_fused"},
    ("heads_1032", 32, 16): {"heads_unfused_nf"},
    ("std", 32, 1): {"heads_fused", "heads_even_outputs"},
    ("std", 32, 15): {"heads_fused", "heads_even_outputs"},
    ("std", 32, 27): {"heads_fused", "heads_32_outputs", "heads_even_outputs"},
    ("std", 32, 28): {"heads_unfused_nc"},
    ("std", 32, 63): {"heads_unfused_nc"},
    ("std", 32, 64): {"heads_unfused_nc", "lsm_lane_stride"},
    ("std", 32, 200): {"heads_unfused_nc", "lsm_lane_stride"},
    ("heads_1024", 32, 27): {"heads_lds_max", "heads_lds_max_backward", "heads_32_outputs"},
}


def test_each_model_labels_what_it_is_listed_for():
    assert set(WANT) == set(CP.MODELS) and len(CP.MODELS) == len(set(CP.MODELS))
    for key in CP.MODELS:
        got = CP.labels_of_model(key)
        assert WANT[key] <= got, (key, sorted(WANT[key] - got))
    # on either side of the edges of cnet_heads_fused_eligible
    assert "heads_fused" not in CP.labels_of_model(("std", 32, 28)) and "heads_unfused_nf" not in CP.labels_of_model(("std", 32, 28))
    assert "heads_fused" not in CP.labels_of_model(("heads_1032", 32, 16)) and "heads_unfused_nc" not in CP.labels_of_model(("heads_1032", 32, 16))
    assert "heads_even_outputs" not in CP.labels_of_model(("std", 32, 16))   # 21 outputs: the pair loop's odd tail
    # the 64 / 65 classes of the lane-strided LogSoftMax kernels
    assert {k[2] + 1 for k in CP.MODELS} >= {2, 16, 17, 28, 29, 64, 65, 201}


def test_a_label_reached_by_one_table_only_is_lost_with_it():
    """every required label that a single model reaches: the tables without that model fail the check above"""
    reach = {lab: [k for k in CP.MODELS if lab in CP.labels_of_model(k)] for lab in CP.REQUIRED}
    assert all(reach.values())
    unique = {lab: ks[0] for lab, ks in reach.items() if len(ks) == 1}
    assert {"fold_launch", "heads_on_input", "one_layer",
            "three_layers", "ragged_width", "flat_fold"} <= set(unique), sorted(unique)
    for lab, key in unique.items():
        rest = [k for k in CP.MODELS if k != key]
        assert not CP.REQUIRED <= CP.labels_of_tables(rest), (lab, key)


def test_the_split_rule():
    """gemm_f32 at the sizes the issue's table names: D = 1152 gives 4 slabs (the consumer folds them), D = 2304 gives 9 (a
    fold launch), K < 512 none; the 512-wide layers give 2 slabs to the layer behind (forward) and below (backward)."""
    for R in CP.ROWS_FULL:
        assert CP.gemm_splits(R, 48, 1152) == 4 and CP.fold_state(R, 48, 1152, True) == "consumer"
        assert CP.gemm_splits(R, 48, 2304) == 9 and CP.fold_state(R, 48, 2304, True) == "launch"
        assert CP.gemm_splits(R, 32, 48) == 1
    for R in CP.ROWS_SHORT:
        assert CP.gemm_splits(R, 512, 1152) == 4    # bn_last layer 0: the flat kernel folds
        assert CP.gemm_splits(R, 40, 512) == 2      # bn_last layer 1: the BN kernel folds
        assert CP.gemm_splits(R, 48, 512) == 2      # wide_second: layer 1's input gradient
        assert CP.fold_state(R, 48, 512, False) == "launch"
    # no table reaches the split form of the large Linear (out of scope here: tests/test_gpu_widths.py)
    assert CP.gemm_splits(64, 4096, 4096) == 16


def test_the_row_lists_bracket_every_row_threshold():
    full, short = set(CP.ROWS_FULL), set(CP.ROWS_SHORT)
    keep = CP.FB_RG * CP.FB_KEEP
    assert {keep - 1, keep, keep + 1} <= full and {CP.FB_RG - 1, CP.FB_RG, CP.FB_RG + 1} <= full
    assert {CP.BN_RG - 1, CP.BN_RG, CP.BN_RG + 1} <= full and {1, 2, 3} <= full
    assert max(full) > 2 * keep                        # a thread of the tall branch walks more than two rows
    assert any(R > keep for R in short) and any(R % 4 for R in short) and 1 in short
    assert CP.rows_keep(keep) and not CP.rows_keep(keep + 1)
    for key in CP.MODELS:
        assert set(CP.rows_of(key)) in (full, short)
    assert set(CP.EVAL_ROWS) | set(CP.DRAW_ROWS) | set(CP.DET_ROWS) <= full
    # deterministic mode: the heads' launch leaves the top activation to its own kernel, the weight gradients stay on the chain
    det = CP.labels_of_case(("std", 32, 16), 5, deterministic=True)
    assert "top_act_in_heads" not in det and "heads_fused" in det
    assert "dgrad_fold_deferred" not in CP.labels_of_case(("wide_second", 32, 16), 5, wgrad_async=False)
    assert "bn_separate" in CP.labels_of_case(("std", 32, 16), 5, fuse=False)


def test_every_case_has_inputs_of_its_shapes():
    assert len(CP.cases()) == len(set(CP.cases()))
    for key, R in CP.cases():
        if R > 5:
            continue
        c = CP.inputs(key, R, CP.seed_of(key, R))
        table, L, cc = key
        assert c["x"].shape == c["x2"].shape == (R, 36 * L) and c["gb"].shape == (R, 4) and c["gc"].shape == (R, cc + 1)
        assert [None if m is None else m.shape for m in c["masks"]] == [(R, n) if p > 0 else None for n, bn, p in CP.TABLES[table]]
    for k in CP.SEED_OVERRIDES:
        assert (k[:3], k[3]) in CP.cases(), k


def test_keep_mask_restatement():
    """splitmix64's published first outputs of the state 0 (output k mixes k + 1 increments; the restatement adds one itself),
    and the draw's shape: float32 0 / 1, a share 1 - p kept, streams that differ, a seed that wraps"""
    gamma = 0x9E3779B97F4A7C15
    z = np.array([0, gamma, (2 * gamma) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    assert [int(v) for v in CP.splitmix64(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    m = CP.keep_mask(0, 1 << 16, 0.5)
    assert m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0} and abs(m.mean() - 0.5) < 0.01
    assert m[0] == 1.0   # 0xE220A8 / 2^24 = 0.883 is not below 0.5
    assert abs(CP.keep_mask(3, 1 << 16, 0.25).mean() - 0.75) < 0.01
    assert (CP.keep_mask(1, 4096, 0.5) != CP.keep_mask(2, 4096, 0.5)).mean() > 0.4
    big = (1 << 63) + 12345   # seed * 0x100000001B3 wraps
    assert np.array_equal(CP.keep_mask(big, 8, 0.5), CP.keep_mask(big, 16, 0.5)[:8])
    assert CP.keep_mask(big, 4096, 0.5).mean() > 0.4
