"""Soft-NMS without a GPU: the setting's validation (nms_settings), the restatement of tests/soft_nms_ref.py against the oracle's
NMS (method hard) and against itself (fp32 against float64 on margin-filtered cases), the case builder of the GPU test reaching
its quota, and a static check of the Lua drop-in's call."""
import math
import os
import re

import numpy as np
import pytest

import soft_nms_ref as R
from test_abi import ROOT, _lua_code

SHAPES = (1, 2, 63, 64, 65, 257, 512, 513, 1000, 2048, 2049)     # the GPU test's counts for the inexact combinations


def _nms_settings():
    from frcnn_amd.Detector import nms_settings
    return nms_settings


def test_nms_settings_defaults_and_accepted_tables():
    ns = _nms_settings()
    assert ns(None) == ("hard", 0.1, 0.5, 0.001, False)
    assert ns({}) == ns(None) == ns(dict(class_count=16)) == ns(dict(class_count=16, nms=None))
    assert ns(dict(method="hard")) == ("hard", 0.1, 0.5, 0.001, False)
    assert ns(dict(method="hard", overlap=0.3)) == ("hard", 0.3, 0.5, 0.001, True)
    assert ns(dict(nms=dict(method="gaussian", sigma=0.25), class_count=16)) == ("gaussian", 0.1, 0.25, 0.001, False)
    assert ns(dict(method="linear", overlap=1, min_score=0)) == ("linear", 1.0, 0.5, 0.0, True)
    assert ns(dict(method="linear", overlap=np.float32(0.5), sigma=np.float64(2), min_score=np.float32(0.5)))[1:4] == (0.5, 2.0, 0.5)


@pytest.mark.parametrize("table", [
    dict(metod="hard"), dict(method="hard", top=3), dict(method="soft"), dict(method=1), dict(method=None), dict(method=True),
    dict(overlap=True), dict(sigma=False), dict(min_score=True), dict(overlap="0.3"), dict(sigma=None), dict(min_score=[0.1]),
    dict(overlap=0), dict(overlap=0.0), dict(overlap=-0.1), dict(overlap=1.01), dict(overlap=float("nan")),
    dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
    dict(min_score=-0.001), dict(min_score=1), dict(min_score=1.0), dict(min_score=float("nan")),
    "gaussian", 3, ["gaussian"],
])
def test_nms_settings_rejects(table):
    with pytest.raises(ValueError):
        _nms_settings()(table)
    if isinstance(table, dict):
        with pytest.raises(ValueError):
            _nms_settings()(dict(class_count=16, nms=table))


def test_detector_takes_the_setting_from_the_argument_or_the_cfg():
    """Detector.set_nms is host code: validated before any device call"""
    from frcnn_amd.Detector import Detector
    d = Detector.__new__(Detector)
    d.set_nms(dict(class_count=16))
    assert (d.nms_method, d.nms_overlap, d.nms_sigma, d.nms_min_score) == ("hard", 0.1, 0.5, 0.001)
    d.set_nms(dict(method="gaussian", min_score=0))
    assert (d.nms_method, d.nms_min_score) == ("gaussian", 0.0)
    with pytest.raises(ValueError):
        d.set_nms(dict(method="gaussian", sigma=0))
    assert d.nms_method == "gaussian"
    assert Detector.nms_settings(dict(method="linear"))[0] == "linear"
    # Detector(model, nms=...) refuses a bad table before it looks at the model, let alone the device
    for bad in (dict(method="soft"), dict(sigma=0), "gaussian"):
        with pytest.raises(ValueError):
            Detector(None, nms=bad)


# ------------------------------------------------------------------------------------------------ the restatement
def _exact_inputs(kind, rng, n):
    """the GPU test's generators (tests/test_gpu_soft_nms.py imports them from here): rows n x 5, probabilities in column 5"""
    if kind == "clustered":
        return R.rows5(R.clustered_boxes(rng, n), np.round(rng.rand(n) * 64) / 64 * 0.9 + 0.05)
    if kind == "disjoint":
        return R.rows5(R.disjoint_boxes(rng, n), rng.rand(n) * 0.9 + 0.05)
    if kind == "same_box":
        return R.rows5(R.same_box(rng, n), rng.rand(n) * 0.9 + 0.05)
    if kind == "equal_scores":
        return R.rows5(R.clustered_boxes(rng, n), np.full(n, 0.5))
    rows = R.rows5(R.clustered_boxes(rng, n), rng.rand(n) * 0.9 + 0.05)
    if n:
        if kind == "one_nan":
            rows[rng.randint(n), 4] = np.nan
        elif kind == "one_neg_inf":
            rows[rng.randint(n), 4] = -np.inf
        elif kind == "below_min_score":
            rows[rng.rand(n) < 0.5, 4] = 0.0005
        else:
            raise KeyError(kind)
    return rows


KINDS = ("clustered", "disjoint", "same_box", "equal_scores", "one_nan", "one_neg_inf", "below_min_score")


def exact_inputs(kind, seed, n, log_domain):
    rows = _exact_inputs(kind, np.random.RandomState(seed), n)
    if log_domain:
        inf = np.isinf(rows[:, 4])
        with np.errstate(all="ignore"):
            rows[:, 4] = np.log(rows[:, 4])        # (fp32 log of an fp32 probability)
        rows[inf, 4] = -np.inf                     # (the -inf row stays one)
    return rows


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "one_nan"])
def test_hard_restatement_equals_the_oracle_nms_keyed_by_the_score(O, kind):
    """method hard with nothing below min_score is nms(rows, Nt, score column): the same arithmetic, the same tie rule"""
    for n in (1, 2, 63, 64, 65, 257):
        for Nt in (0.1, 0.5):
            rows = exact_inputs(kind, 11 * n + 1, n, 0)
            pick, out = R.soft_nms_f32(rows, 5, R.HARD, Nt, 0.5, -np.inf, 0)
            assert pick.tolist() == O.nms(rows, Nt, 2, 5).tolist(), (kind, n, Nt)
            assert np.array_equal(out.view(np.uint32), rows[pick - 1, 4].view(np.uint32))
            # per class: a stable partition of the one-pass picks is the per-class result
            cls = np.random.RandomState(n).randint(1, 4, n)
            pick, _ = R.soft_nms_f32(rows, 5, R.HARD, Nt, 0.5, -np.inf, 0, cls)
            for c in (1, 2, 3):
                sub = np.nonzero(cls == c)[0]
                want = sub[O.nms(rows[sub], Nt, 2, 5) - 1] + 1 if len(sub) else np.zeros(0, np.int64)
                assert pick[cls[pick - 1] == c].tolist() == want.tolist(), (kind, n, Nt, c)


def test_restatement_edges():
    f = R.soft_nms_f32
    assert f(np.zeros((0, 5), np.float32), 5, R.GAUSSIAN, 0.3, 0.5, 0.001, 0)[0].shape == (0,)
    rows = exact_inputs("one_nan", 3, 65, 0)
    bad = int(np.nonzero(np.isnan(rows[:, 4]))[0][0])
    for method in (R.HARD, R.LINEAR, R.GAUSSIAN):
        pick, out = f(rows, 5, method, 0.3, 0.5, -np.inf, 0)
        assert bad + 1 not in pick.tolist() and not np.isnan(out).any()
        assert np.all(np.diff(out) <= 0), "the scores at pick never increase"
    rows = exact_inputs("below_min_score", 4, 257, 0)
    pick, _ = f(rows, 5, R.GAUSSIAN, 0.3, 0.5, 0.001, 0)
    assert not np.any(rows[pick - 1, 4] < 0.001)
    rows = exact_inputs("disjoint", 5, 257, 0)
    for method in (R.HARD, R.LINEAR, R.GAUSSIAN):
        pick, out = f(rows, 5, method, 0.3, 0.5, 0.001, 0)
        order = np.lexsort((-np.arange(257), -rows[:, 4]))
        assert pick.tolist() == (order + 1).tolist() and np.array_equal(out, rows[order, 4])
    # ties go to the higher row, -0 equals +0
    rows = R.rows5(R.disjoint_boxes(np.random.RandomState(1), 4), [0.0, -0.0, 0.0, -1.0])
    assert f(rows, 5, R.GAUSSIAN, 0.3, 0.5, -np.inf, 1)[0].tolist() == [3, 2, 1, 4]


@pytest.mark.parametrize("method,log_domain", [(m, l) for m in (R.HARD, R.LINEAR, R.GAUSSIAN) for l in (0, 1)])
def test_fp32_and_float64_restatements_pick_the_same_rows_on_margin_filtered_cases(method, log_domain):
    P = R.INEXACT_PARAMS[(R.LINEAR, 1) if log_domain else (R.GAUSSIAN, 0)]
    kept = 0
    for n in (2, 63, 65, 257):
        for seed in range(6):
            rng = np.random.RandomState(100 * n + seed)
            rows = R.rows5(R.sparse_clusters(rng, n), R.grid_scores(rng, n, -1.6, -0.01) if log_domain else R.grid_scores(rng, n, 0.05, 1.0))
            cls = None if seed % 2 else rng.randint(1, 4, n)
            p64, s64, st = R.soft_nms_f64(rows, 5, method, P["overlap"], P["sigma"], P["min_score"], log_domain, cls)
            # the fp32 restatement's error is within the device's bound (its exp / log1p are numpy's fp32 ones, 1 ULP class); the
            # exact combinations carry roundings too on this side: grant them the gaussian / linear bound of the same run
            bound = max(R.score_error_bound(R.GAUSSIAN, 0, P["sigma"], st), R.score_error_bound(R.LINEAR, 1, P["sigma"], st))
            if not st["margin"] > 2.0 * bound:
                continue
            kept += 1
            p32, s32 = R.soft_nms_f32(rows, 5, method, P["overlap"], P["sigma"], P["min_score"], log_domain, cls)
            assert p32.tolist() == p64.tolist(), (method, log_domain, n, seed)
            err = np.abs(s32.astype(np.float64) - s64)
            if not log_domain:
                err = err / np.maximum(np.abs(s64), np.finfo(np.float64).tiny)
            assert np.all(err <= bound), (method, log_domain, n, seed, float(err.max()), bound)
    assert kept >= 12, kept


@pytest.mark.parametrize("method,log_domain", R.INEXACT)
def test_case_builder_of_the_gpu_test_reaches_its_quota(method, log_domain):
    """inexact_cases asserts its own cap (at most half of the seeds it tries are discarded); every shape of the GPU test"""
    for n in SHAPES:
        for nclasses in (0, 3):
            quota = 1 if n > 1000 else R.INEXACT_QUOTA
            cases = R.inexact_cases(method, log_domain, n, nclasses, quota)
            assert len(cases) == quota
            for c in cases:
                assert c["stats"]["margin"] > 2.0 * c["bound"] >= 2.0 * R.U and math.isfinite(c["bound"])
    assert R.is_exact(R.HARD, 0) and R.is_exact(R.HARD, 1) and R.is_exact(R.LINEAR, 0) and R.is_exact(R.GAUSSIAN, 1)
    assert not R.is_exact(R.LINEAR, 1) and not R.is_exact(R.GAUSSIAN, 0)


# ------------------------------------------------------------------------------------------------ the Lua drop-in, statically
def _split_args(text):
    """the top-level comma-separated arguments of a call whose opening parenthesis is text[0]"""
    depth, args, cur = 0, [], []
    for ch in text:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append("".join(cur).strip())
                return args
        if ch == "," and depth == 1:
            args.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    raise AssertionError("unbalanced call")


def test_lua_drop_in_calls_soft_nms_with_the_headers_argument_count():
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+frcnn_soft_nms_batch\s*\(", hdr)
    assert m, "frcnn_soft_nms_batch is not declared"
    declared = _split_args(hdr[m.end() - 1:])
    assert len(declared) == 20
    from frcnn_amd import _lib
    assert len(_lib._SIGS["frcnn_soft_nms_batch"][0]) == len(declared)
    det = _lua_code(open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read())
    calls = [c.end() for c in re.finditer(r"C\.frcnn_soft_nms_batch\s*\(", det)]
    assert len(calls) == 1, "Detector_hip.lua must call frcnn_soft_nms_batch once"
    assert len(_split_args(det[calls[0] - 1:])) == len(declared)
    assert "C.frcnn_soft_nms_workspace_bytes" in det and "function Detector.nms_settings" in det and "cfg.nms" in det
    shim = _lua_code(open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read())
    calls = [c.end() for c in re.finditer(r"C\.frcnn_soft_nms_batch\s*\(", shim)]
    assert len(calls) == 1 and len(_split_args(shim[calls[0] - 1:])) == len(declared)
    assert "function M.soft_nms" in shim
    assert re.search(r"^soft_nms = hip\.soft_nms", open(os.path.join(ROOT, "bindings", "nms.lua")).read(), re.M)
