"""The tables of tests/test_gpu_gemm_plans.py reach every launch plan of the two Linear products they exist for
(tests/gemm_plan.py restates the host-side shape rules of csrc/gemm.hip gemm_f32 and csrc/gemmx.hip gx_plan / gx_run; no GPU
needed).  A later edit of the tables cannot drop a branch without this failing."""
import numpy as np
import pytest

import cnet_plan as NP
import convx_plan as XP
import gemm_plan as GP
import width_plan as WP


def test_restatement_of_gemm_f32_at_known_values():
    """values worked out by hand from gemm.hip gemm_f32 for the three products of Linear(R, I, O)"""
    def f(role, shape, **kw):
        p = GP.f32_plan(role, shape, **kw)
        return p["TNs"], p["splitK"], p["last"], "dma" if p["dma"] else "reg%d%d" % (p["av"], p["bv"]), p["where"]
    # 128-column tiles need N >= 2048 and K >= 512; 9 slabs of 256; 8 slabs of 288 with 34 left; O % 4 != 0: scalar loads of gY
    assert f("forward", (5, 2304, 2050)) == (128, 9, 256, "dma", "fold_bias")
    assert f("input_gradient", (5, 2304, 2050)) == (128, 8, 34, "reg01", "fold")
    assert f("weight_gradient", (5, 2304, 2050)) == (64, 1, 5, "reg01", "tile_accumulate")
    assert f("forward", (600, 2052, 520)) == (64, 8, 36, "dma", "fold_bias")
    assert f("input_gradient", (600, 2052, 520)) == (128, 2, 232, "dma", "fold")
    assert f("weight_gradient", (600, 2052, 520)) == (128, 2, 280, "dma", "fold_accumulate")
    # 16 estimated, 288 values per split, 15 slabs, 68 left; the bbox head's K = 4 and M = 4
    assert f("forward", (65, 4100, 4)) == (64, 15, 68, "dma", "fold_bias")
    assert f("input_gradient", (65, 4100, 4)) == (64, 1, 4, "reg11", "tile_store")
    assert f("weight_gradient", (65, 4100, 4)) == (64, 1, 65, "dma", "tile_accumulate")
    assert f("weight_gradient", (1030, 68, 36)) == (64, 4, 166, "dma", "fold_accumulate")
    assert f("forward", (64, 60, 64)) == (64, 1, 60, "reg11", "tile_store")
    assert f("forward", (64, 60, 64), a_aligned=False) == (64, 1, 60, "reg01", "tile_store")
    assert f("forward", (64, 60, 64), b_aligned=False) == (64, 1, 60, "reg10", "tile_store")
    assert f("forward", (3, 8200, 65)) == (64, 16, 40, "dma", "fold_bias")
    assert f("weight_gradient", (513, 2048, 20)) == (128, 2, 225, "dma", "fold_accumulate")
    # the DMA kernel needs dword-aligned addresses only: a 4-byte offset changes nothing where it is taken
    assert f("forward", (600, 2052, 520), a_aligned=False, b_aligned=False) == (64, 8, 36, "dma", "fold_bias")
    # Linear(13824, 1024) at 138 rows, the fp32 products of a training step below the split form's row count
    assert f("forward", (138, 13824, 1024)) == (64, 16, 864, "dma", "fold_bias")
    p = GP.f32_plan("forward", (1665, 768, 1666))
    assert (p["by_k"], p["by_slots"], p["splitK"], p["kPerSplit"]) == (3, 2, 2, 384)
    # tests/test_gpu_elem.py::test_linear_forward_backward, the four shapes gemm_f32 had at operator level: what they reach
    old = set()
    for shape in ((7, 100, 33), (96, 864, 48), (130, 13824, 64), (1, 512, 17)):
        for role in GP.ROLES:
            old |= GP.f32_labels(GP.f32_plan(role, shape))
    assert not {"tn128_dma", "tn128_reg", "ep_fold_accumulate", "last_split_short"} & old
    assert GP.REG_VARIANTS & old == {"reg_kn_01", "reg_kn_11", "reg_mn_01"}


def test_split_plan_is_the_one_of_the_classification_net_tables():
    for M, N, K in ((5, 2050, 2304), (65, 4, 4100), (1665, 1666, 768), (36, 68, 1030), (1, 1, 1)):
        s = NP.gemm_split_plan(M, N, K)
        assert s["splitK"] == NP.gemm_splits(M, N, K) and s["kPerSplit"] % NP.GBK == 0
        assert (s["splitK"] - 1) * s["kPerSplit"] < K <= s["splitK"] * s["kPerSplit"]


def test_restatement_of_gx_plan_at_known_values():
    """tile heights and splits of the shapes the tables were made from (gemmx.hip gx_plan's cost model by hand)"""
    def g(role, shape, tm=None):
        p = GP.gx_launch(role, shape, 1, tm)
        return p["TM"], p["splitK"], p["last"], p["blocks"]
    assert g("forward", (270, 13824, 272)) == (64, 25, 384, 250)
    assert g("forward", (2000, 1040, 496)) == (64, 4, 224, 256)
    # the weight gradient: one slab per 1024 rows of k, whatever the cost model says -- 2000 rows: two slabs of 1008 and 992
    assert g("weight_gradient", (2000, 1040, 496)) == (64, 2, 992, 80)
    assert [g("weight_gradient", (R, 1040, 1024))[1] for R in (1024, 1025, 2048, 2049)] == [1, 2, 2, 3]
    assert g("forward", (250, 2048, 2064)) == (64, 7, 224, 252)
    assert g("input_gradient", (250, 2048, 2064))[:3] == (64, 4, 480)
    assert g("input_gradient", (40, 3088, 8208))[:3] == (64, 4, 2016) and GP.gx_launch("input_gradient", (40, 3088, 8208), 1)["kPerSplit"] == 2064
    assert g("forward", (1131, 13824, 64))[:2] == (64, 28)
    # R = 32 / 33 pad to 32 / 48 rows of k
    assert [GP.gx_launch("weight_gradient", (R, 13824, 2304), 1)["K"] for R in (32, 33)] == [32, 48]
    assert g("weight_gradient", (32, 13824, 2304))[:2] == (128, 1)
    # a forced height: every role that has it takes it; 256 rows exist for planes x planes only, the others keep their own choice
    for tm in (64, 128, 192):
        assert [g(role, (385, 1648, 1584), tm)[0] for role in GP.ROLES] == [tm] * 3
    assert [g(role, (385, 1648, 1584), 256)[:2] for role in GP.ROLES] == [(64, 5), (64, 4), (256, 1)]
    assert [g(role, (385, 1648, 1584))[:2] for role in GP.ROLES[:2]] == [(64, 5), (64, 4)]
    # ring depths (gx_ring): planes x planes, three bf16 planes / two fp16 planes
    assert [GP.gx_ring(tm, 0, 3) for tm in (64, 128, 192, 256)] == [2, 2, 3, 3]
    assert [GP.gx_ring(tm, 0, 2) for tm in (64, 128, 192, 256)] == [3, 3, 4, 4]
    assert [GP.gx_ring(tm, 1, 3) for tm in (64, 128, 192)] == [3, 2, 4] and [GP.gx_ring(tm, 2, 2) for tm in (64, 128, 192)] == [3, 3, 4]
    assert [GP.linear_x_rows_padded(R) for R in (1, 16, 17, 32, 33)] == [16, 16, 32, 32, 48]


def test_eligibility_with_the_option_mask():
    for shape in ((270, 13824, 272), (31, 13824, 4096), (32, 13824, 2304), (560, 13824, 1024), (560, 13820, 1024), (100, 100, 100)):
        for role in (1, 2, 4):
            assert GP.linear_x_eligible(role, *shape) == WP.linear_x_eligible(role, *shape)      # mask -1: the built-in rule
            assert not GP.linear_x_eligible(role, *shape, mask=0)
            assert not GP.linear_x_eligible(role, *shape, mask=7, split_bf16=False)
    assert [GP.linear_x_eligible(r, 32, 13824, 2304, mask=7) for r in (1, 2, 4)] == [True] * 3
    assert [GP.linear_x_eligible(r, 32, 13824, 2304) for r in (1, 2, 4)] == [False, True, False]
    assert [GP.linear_x_eligible(r, 560, 13824, 1024, mask=5) for r in (1, 2, 4)] == [True, False, True]
    assert not GP.linear_x_eligible(1, 31, 13824, 4096, mask=7) and not GP.linear_x_eligible(1, 560, 13820, 1024, mask=7)


def test_case_names_are_unique_and_cases_are_small():
    names = [c["name"] for c in GP.F32_CASES] + ["x_" + c["name"] for c in GP.GX_CASES]
    assert len(names) == len(set(names))
    for c in GP.F32_CASES:
        R, I, O = c["shape"]
        assert R * I * O <= 2.2e9 and set(c["placings"]) <= set(GP.PLACINGS) and set(c["roles"]) <= set(GP.ROLES), c["name"]
    for c in GP.GX_CASES:
        R, I, O = c["shape"]
        assert R * I * O <= 1.3e9 and c["placing"] in GP.PLACINGS, c["name"]


def test_every_split_case_is_eligible_and_no_fp32_case_is():
    """gemm_x_roles = 7 sends all three roles of every gemmx case to gemm_planes_kernel; the gemm_f32 cases run with
    gemm_x_roles = 0"""
    for c in GP.GX_CASES:
        for role in GP.ROLES:
            assert GP.linear_x_eligible(GP.ROLE_BIT[role], *c["shape"], mask=7), (c["name"], role)
    for c in GP.F32_CASES:
        for role in GP.ROLES:
            assert not GP.linear_x_eligible(GP.ROLE_BIT[role], *c["shape"], mask=0)


def test_cases_reach_what_they_are_listed_for():
    for c in GP.F32_CASES:
        labels = set()
        for r in GP.f32_runs([c]):
            labels |= GP.f32_labels_of_run(r)
        assert c["want"] and c["want"] <= labels, (c["name"], sorted(c["want"] - labels))
    for c in GP.GX_CASES:
        labels = set()
        for r in GP.gx_runs([c]):
            labels |= GP.gx_labels_of_run(r)
        assert c["want"] and c["want"] <= labels, (c["name"], sorted(c["want"] - labels))


def _reached(f32_cases, gx_cases):
    """label -> the cases that reach it"""
    out = {}
    for r in GP.f32_runs(f32_cases):
        for l in GP.f32_labels_of_run(r):
            out.setdefault(l, set()).add(r["name"])
    for r in GP.gx_runs(gx_cases):
        for l in GP.gx_labels_of_run(r):
            out.setdefault(l, set()).add("x_" + r["name"])
    return out


def _missing(f32_cases, gx_cases):
    got = _reached(f32_cases, gx_cases)
    return sorted(l for l in GP.REQUIRED if not got.get(l))


def test_tables_reach_every_required_label():
    """gemm_f32: both tile widths in both kernels, the split ranges, both caps, K tails, the three DMA orientations, the twelve
    reachable register variants, every epilogue, the edge sizes of M and N.  gemmx: per role, and per form where the form
    decides (ring depth, block count): every case runs every role in both forms."""
    assert _missing(GP.F32_CASES, GP.GX_CASES) == []
    assert len(GP.REG_VARIANTS) == 12 and GP.REG_VARIANTS <= GP.F32_REQUIRED
    for form in GP.FORMS.values():
        for l in ("blocks_mod8", "blocks_lt_8", "fwd", "dgrad", "wgrad"):
            assert "%s:%s" % (form, l) in GP.GX_REQUIRED


def test_removing_a_case_that_a_label_depends_on_is_noticed():
    got = _reached(GP.F32_CASES, GP.GX_CASES)
    single = {l: next(iter(got[l])) for l in sorted(GP.REQUIRED) if len(got[l]) == 1}
    # labels that rest on one case each (two of them: the slot cap of gemm_f32's split estimate; gemm_planes_kernel's weight
    # gradient with two K steps)
    assert single["splits_capped_by_slots"] == "capped_by_slots" and single["wgrad:rp_32"] == "x_rp_32"
    assert {"reg_kk_10", "reg_kk_01", "tn128_reg", "k_tail_last_split_reg", "f16x3:blocks_lt_8", "dgrad:n_mod256_240"} <= set(single)
    for label, name in single.items():
        f32 = [c for c in GP.F32_CASES if c["name"] != name]
        gx = [c for c in GP.GX_CASES if "x_" + c["name"] != name]
        assert len(f32) + len(gx) == len(GP.F32_CASES) + len(GP.GX_CASES) - 1
        assert label in _missing(f32, gx), (label, name)
    # a variant list emptied: the placings of short_k pick three of the four k-contiguous register variants
    trimmed = [dict(c, placings=("aligned",)) if c["name"] == "short_k" else c for c in GP.F32_CASES]
    assert {"reg_kk_10", "reg_kk_01"} <= set(_missing(trimmed, GP.GX_CASES))
    # the wide-range run of the gemmx part
    assert "wide_range" in _missing(GP.F32_CASES, [dict(c, wide=False) for c in GP.GX_CASES])


@pytest.mark.parametrize("wide", [False, True], ids=["decades", "twelve_binades"])
def test_representation_share_covers_the_inputs_of_the_gpu_file(wide):
    """both splits emulated in numpy on inputs drawn as the GPU file draws them, the kept plane products summed in fp64: the
    distance to the fp64 product stays inside convx_plan.representation_bound in all three roles -- with the twelve binades of
    the wide run the low fp16 plane loses bits, and the 2^-38 amax term of the bound is what covers them"""
    x, w, b, gy, gw0, gb0 = GP.linear_inputs(np.random.RandomState(5), (48, 208, 96), wide)
    ops = {"forward": (lambda a, c: a @ c.T, x, w), "input_gradient": (lambda a, c: a @ c, gy, w),
           "weight_gradient": (lambda a, c: a.T @ c, gy, x)}
    for role, (op, a, c) in ops.items():
        want = op(a.astype(np.float64), c.astype(np.float64))
        for form in GP.FORMS:
            err = np.abs(XP.emulate_split(op, a, c, form) - want)
            rep = XP.representation_bound(op, a, c, form)
            assert np.all(err <= rep), (role, form, float((err / np.maximum(rep, 1e-300)).max()))
    if wide:   # twelve binades and more
        for a in (x, gy):
            m = np.abs(a[a != 0])
            assert np.log2(m.max() / np.median(m)) >= 6 and np.log2(m.max() / m.min()) >= 12
