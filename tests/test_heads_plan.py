"""The tables of tests/test_gpu_heads_chain.py reach every path of the anchor nets' sparse chain they exist for, and the fp64
references they are compared with are right: tests/heads_plan.py restates the host-side rules of csrc/heads.hip
(heads_plan_splits, heads_add_job, hd_grid) and csrc/gemm.hip (gemm_f32_group); no GPU needed.  The references are anchored
independently of the implementation: the sparse forward equals a plain fp64 valid convolution, PReLU and 1 x 1 convolution on the
whole map read at the positions, the sparse backward equals the dense backward pass with a delta map that is zero elsewhere,
and every exact-data case meets its exactness condition on the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import heads_plan as HP
import width_plan as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouped_product_tables_reach_every_required_label():
    reached = set()
    names = set()
    for c in HP.GEMM_CASES:
        assert c["name"] not in names and 1 <= len(c["jobs"]) <= HP.GROUP_MAX
        names.add(c["name"])
        L = HP.group_labels(c)
        assert c["want"] <= L, (c["name"], sorted(c["want"] - L))
        reached |= L
        for j in c["jobs"] if c["role"] is None else []:   # (a chain product has the chain's dimensions: K = n, 18 or P)
            assert j["M"] in (0,) + HP.GEMM_M_N and j["N"] in (0,) + HP.GEMM_M_N and j["K"] in HP.GEMM_K, (c["name"], j)
    assert HP.GEMM_REQUIRED <= reached, sorted(HP.GEMM_REQUIRED - reached)
    # A m-contiguous with B k-contiguous is no product of the chain: it is launched by its own case, and by the chain's GH
    # product when its first net has a single position
    assert [c["name"] for c in HP.GEMM_CASES if "kernel_mk" in HP.group_labels(c)] == ["orient_mk", "p1_first_gh"]


def test_restatement_of_the_grouped_launch_at_known_values():
    """values worked out by hand from gemm.hip gemm_f32_group"""
    assert HP.k_runs(72, 3) == (32, [32, 32, 8]) and HP.k_runs(72, 2) == (64, [64, 8]) and HP.k_runs(33, 2) == (32, [32, 1])
    assert HP.k_runs(64, 3) == (32, [32, 32]) and HP.k_runs(33, 3) == (32, [32, 1])      # a run left empty: refused
    for jobs, what in HP.GEMM_ERRORS:
        bad = not 1 <= len(jobs) <= HP.GROUP_MAX or any(len(HP.k_runs(j["K"], j["splits"])[1]) != j["splits"] for j in jobs)
        assert bad, what
    # the chain's orientations: strides of each product and the kernel a group of them launches
    q = HP.chain_products(65, 72, 63, 3)
    assert HP.strides(q["HX"]) == (72, 1, 1, 72, 63) and HP.strides(q["OUT"]) == (65, 1, 63, 1, 63)
    assert HP.strides(q["GH"]) == (1, 65, 63, 1, 63) and HP.strides(q["DX"]) == (1, 63, 72, 1, 72)
    assert HP.strides(q["gW1"]) == (63, 1, 1, 63, 65) and HP.strides(q["gW"]) == (63, 1, 72, 1, 72)
    assert [HP.group_flags([q[r]]) for r in ("HX", "OUT", "GH", "DX", "gW1", "gW")] == ["kk", "kn", "mn", "mn", "kk", "kn"]
    # P = 1: HY[n][1] and D[18][1] have a unit k stride by accident, GH^T[1][n] a unit k stride as well
    p1 = HP.chain_products(64, 72, 1)
    assert HP.job_flags(p1["OUT"]) == "kk" and HP.job_flags(p1["GH"]) == "mk" and HP.job_flags(p1["DX"]) == "kn"


def test_chain_tables_reach_every_required_label():
    reached = set()
    for c in HP.CHAIN_CASES:
        assert 1 <= len(c["nets"]) <= 4
        L = HP.chain_labels(c)
        assert c["want"] <= L, (c["name"], sorted(c["want"] - L))
        reached |= L
    assert HP.CHAIN_REQUIRED <= reached, sorted(HP.CHAIN_REQUIRED - reached)
    assert not HP.CHAIN_NOT_REACHED & reached
    mixed = HP.find("mixed")["nets"]
    assert [t["k"] for t in mixed] == [3, 3, 5, 7] and all(8 <= t["Cin"] <= 16 for t in mixed)
    assert [t["n"] for t in mixed] == [64, 96, 32, 130] and sorted(t["P"] for t in mixed) == [0, 1, 64, 65]
    assert all(t["H"] - t["k"] <= 9 and t["W"] - t["k"] <= 9 for t in mixed)
    assert HP.find("mixed_p1_first")["nets"][0]["P"] == 1 and HP.find("mixed_p0_first")["nets"][0]["P"] == 0


def test_restatement_of_the_split_planner_at_known_values():
    """heads.hip heads_plan_splits = width_plan.head_splits, by hand for the shapes of the tables"""
    stride, fold = HP.find("stride")["nets"][0], HP.find("fold")["nets"][0]
    assert stride["ckk"] == 2352 and stride["P"] * stride["ckk"] > HP.HD_GRID_CAP * 256
    assert HP.planned_splits(stride) == 8 and HP.k_runs(2352, 8) == (320, [320] * 7 + [112])
    assert HP.planned_splits(fold) == 9 and HP.k_runs(2352, 9) == (288, [288] * 8 + [48])
    assert HP.k_runs(2352, 11) == (224, [224] * 10 + [112])
    for t, what in HP.CHAIN_ERRORS:
        assert len(HP.k_runs(t["ckk"], t["force"])[1]) != t["force"], what
    assert [HP.planned_splits(t) for t in HP.find("mixed")["nets"] if t["P"]] == [1, 1, 3]
    assert HP.k_runs(784, 3) == (288, [288, 288, 208])
    # the model's own shapes (tests/width_plan.py restates the same rule for tests/test_gpu_widths.py)
    assert WP.head_splits(256, 384, 7, 256) == 16 and WP.head_splits(256, 256, 3, 64) == 9


def test_positions_are_distinct_and_inside_and_of_the_kinds_the_issue_names():
    for c in HP.CHAIN_CASES:
        for i, t in enumerate(c["nets"]):
            pos = HP.net_data(c, i)["pos"]
            hw = t["Ho"] * t["Wo"]
            assert pos.dtype == np.int32 and len(pos) == t["P"] == len(set(pos.tolist()))
            assert all(0 <= p < hw for p in pos)
            if t["pos"] == "corners" and t["P"] >= 4:
                assert {0, t["Wo"] - 1, hw - t["Wo"], hw - 1} <= set(pos.tolist())
            if t["pos"] == "corners" and t["P"] > 4:
                assert list(pos) != sorted(pos)
            if t["pos"] == "all":
                assert sorted(pos) == list(range(hw))
            if HP.overlaps_kk(t):   # some element of the input map lies under k k patches
                assert HP.ref_col2im(t, np.zeros((t["P"], t["ckk"])), pos, np.zeros((t["Cin"], t["H"], t["W"])))[2].max() == t["k"] ** 2


def _nets(cases, exact=False):
    return [(c, i) for c in cases for i, t in enumerate(c["nets"]) if t["P"] > 0 and (c["exact"] or not exact)]


@pytest.mark.parametrize("c,i", _nets(HP.CHAIN_CASES), ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_reference_equals_the_dense_net(c, i):
    """the sparse references against a plain fp64 dense convolution net: forward read at the positions, backward with the delta
    map zero elsewhere; and the stage functions compose to the whole"""
    t, d = c["nets"][i], HP.net_data(c, i)
    r = HP.reference(t, d)
    hx, hy, out = HP.dense_forward(t, d)
    hw = t["Ho"] * t["Wo"]
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12)   # noqa: E731  (fp64 sums in another order)
    assert close(r["HX"], hx.reshape(t["n"], hw)[:, d["pos"]]) and close(r["HY"], hy.reshape(t["n"], hw)[:, d["pos"]])
    assert close(r["out_at_pos"], out.reshape(HP.HEAD_OUT, hw)[:, d["pos"]])
    off = np.setdiff1d(np.arange(hw), d["pos"])
    assert not d["delta"][:, off].any() and d["delta"][:, d["pos"]].any()
    g = HP.dense_backward(t, d)
    for name in ("gbias1", "gw1", "gbias3", "gslope", "gw3", "gin"):
        assert close(r[name], g[name]), name
    # stage by stage from the stage before
    S = HP.planned_splits(t)
    sl, mg, runs = HP.ref_slabs(d["w3"], r["COL"], S)
    assert len(runs) == S and close(HP.ref_hx(d["bias3"], sl)[0], r["HX"]) and close(HP.ref_out(d["w1"], r["HY"])[0], r["OUT"])
    assert close(HP.ref_gh(d["w1"], r["D"], r["HX"], d["slope"])[0], r["GH"])
    assert (mg >= np.abs(sl) - 1e-12).all()


@pytest.mark.parametrize("c,i", _nets(HP.CHAIN_CASES, True), ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_exact_data_meets_the_exactness_condition(c, i):
    """every sum of magnitudes of every stage stays below 2^24 quarter units: every partial sum, in any order, is exact in fp32,
    and the reference itself is a multiple of 1/4 that fp32 holds"""
    t, d = c["nets"][i], HP.net_data(c, i, exact=True)
    worst = HP.exact_condition(t, d)
    print("%s net %d: largest sum of magnitudes %.0f quarter units (2^24 = %d)" % (c["name"], i, worst, 2 ** 24))
    assert worst < 2 ** 24
    r = HP.reference(t, d)
    for name, v in r.items():
        v = np.asarray(v, np.float64)
        assert np.array_equal(v * 4, np.round(v * 4)) and np.array_equal(v.astype(np.float32).astype(np.float64), v), name
    assert (r["HX"] <= 0).any() and (r["HX"] > 0).any() and r["GH"].any() and r["DX"].any()   # both PReLU branches, no dead data


def test_grouped_product_references():
    for c in HP.GEMM_CASES:
        for j, d in zip(c["jobs"], HP.gemm_inputs(c)):
            want, mag, ks = HP.gemm_reference(j, d)
            a, b = HP.gemm_layout(j, d["A"], d["B"])
            sAm, sAk, sBk, sBn, ldc = HP.strides(j)
            M, N, K = j["M"], j["N"], j["K"]
            assert a.size == M * K and b.size == K * N and ldc >= N
            if M and N:   # the strides address the layout
                m, n, k = M - 1, N - 1, K - 1
                assert a.ravel()[m * sAm + k * sAk] == d["A"][m, k] and b.ravel()[k * sBk + n * sBn] == d["B"][k, n]
            assert want.shape == mag.shape == ((len(ks), M, N) if j["splits"] > 1 else (M, N)) and sum(ks) == K
            assert np.isnan(d["C0"]).all() or j["add"]


def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_header_and_ctypes_table_agree():
    """include/frcnn_hip_heads.h is included by frcnn_hip.h, declares exactly _lib.HEADS_SIGS, and its two structures have the
    members of _lib.GemmJob / _lib.HeadNet in order; frcnn_hip.h's own list (tests/test_abi.py) does not change"""
    from frcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_heads.h")).read()
    names = set(_lib.HEADS_SIGS)
    assert '#include "frcnn_hip_heads.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names and not names & set(_lib.exported_symbols())
    assert not names & (set(_lib.HARD_SIGS) | set(_lib.LOSS_SIGS) | set(_lib.BOX_SIGS) | set(_lib.CLASSBOX_SIGS))
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in names:
        m = re.search(r"^int %s\(([^;]*)\);" % name, code, re.M)
        assert m and len(m.group(1).split(",")) == len(_lib.HEADS_SIGS[name][0]), name
    for struct, cls in (("frcnn_gemm_job", _lib.GemmJob), ("frcnn_head_net", _lib.HeadNet)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        members = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                members += [w.strip(" *") for w in re.sub(r"^(const )?(long long|float|int)\b", "", decl).split(",")]
        assert [m.rstrip("_") for m in members] == [f[0].rstrip("_") for f in cls._fields_], struct
    if os.path.exists(_lib.SO_PATH):
        lib = ctypes.CDLL(_lib.SO_PATH)
        assert all(hasattr(lib, n) for n in names)
        lib.frcnn_heads_plan_splits.restype = ctypes.c_int
        for n, Cin, k, P in ((64, 48, 7, 512), (64, 48, 7, 64), (130, 16, 7, 64), (256, 384, 7, 256), (96, 12, 3, 1), (24, 20, 7, 4096)):
            assert lib.frcnn_heads_plan_splits(n, Cin * k * k, P) == WP.head_splits(n, Cin, k, P), (n, Cin, k, P)
    # the contract the issue asks the header to state
    for word in ("DISTINCT", "duplicate would count its gradient twice", "Untouched", "Scratch, owned by the caller",
                 "5 launches", "7 launches, 5 when no net has a gin", "SKIPPED"):
        assert word in hdr, word
