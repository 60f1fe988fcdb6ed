"""The tables of tests/test_gpu_compact_ops.py reach every edge of the channel-compact launches they exist for, and the numpy
restatement of the gather and the scatter they are compared with is right (tests/compact_plan.py; no GPU needed).  A later edit
of the tables cannot drop the last case of a label without this failing.  Also: the representation share of the GPU file's
error bound with the FULL weight tensor's magnitude, checked against both splits emulated on the gathered operands, and shown to
stay under the project's bar when a dropped filter is 2^10 times larger than the kept ones; the header, the ctypes table and
the build script name the same entry points."""
import os
import re

import numpy as np
import pytest

import compact_plan as KP
import conv_plan as CP
import convx_plan as XP
import width_plan as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sizes_follow_plan_compact():
    assert [KP.sizes(128, nk) for nk in KP.KEPT_COUNTS[128]] == [(64, 16), (64, 16), (64, 16), (64, 32), (64, 64), (64, 64),
                                                                 (128, 80), (128, 112)]
    assert [KP.sizes(192, nk) for nk in KP.KEPT_COUNTS[192]] == [(128, 80), (192, 176)]
    assert KP.sizes(192, 65)[1] // XP.CX_CH == 5
    for C, counts in KP.KEPT_COUNTS.items():
        for nk in counts:   # every count of the issue's list is a block the model runs compact, and some case has it
            assert WP.compact_plan([KP.CIN, C], 1, nk) == "compact", (C, nk)
            assert any(c["C"] == C and c["nk"] == nk and set(c["roles"]) == set(KP.ROLES) for c in KP.CASES), (C, nk)
    assert WP.compact_plan([KP.CIN, 128], 1, 113) == "skipped"          # nkK == C: nothing to leave out


def test_cases_are_compact_blocks_and_small():
    names = [c["name"] for c in KP.CASES]
    assert len(names) == len(set(names))
    for c in KP.CASES:
        cin = KP.WIDE_CIN.get(c["name"], KP.CIN)
        assert KP.eligible(c["C"], c["nk"], c["nb"], cin), c["name"]
        assert WP.compact_plan([cin, c["C"]], 1, c["nk"]) == "compact", c["name"]
        H, W = c["hw"]
        assert H * W <= 2000 and max(c["C"], c["nb"], cin) <= 192, c["name"]
        if set(c["roles"]) & set(KP.CONV_ROLES):
            assert H * W <= 12 * 16, c["name"]
    assert {c["hw"] for c in KP.CASES} >= set(KP.MAPS.values())
    for r in KP.runs():
        L = KP.launch_of_run(r)
        if r["role"] in KP.CONV_ROLES:
            XP.x3_plan(L["shape"], post=r["post"])       # asserts that the launch takes the split form
        else:
            XP.wgradx_plan(L["shape"])


def test_kept_sets():
    for C, nk in ((128, 1), (128, 65), (192, 176)):
        for kind in KP.KINDS:
            if kind == "ends" and nk < 2:
                continue
            k = KP.kept_set(C, nk, kind)
            assert len(k) == nk == len(set(k)) and k == sorted(k) and 0 <= k[0] and k[-1] < C
            t = KP.table(C, k)
            assert t.dtype == np.int32 and list(t[:nk]) == k and (t[nk:] == -1).all() and len(t) == C
    assert KP.kept_set(128, 5, "first") == [0, 1, 2, 3, 4] and KP.kept_set(128, 2, "last") == [126, 127]
    e = KP.kept_set(192, 65, "ends")
    assert e[0] == 0 and e[-1] == 191
    assert KP.kept_set(128, 65, "random") != KP.kept_set(128, 65, "random", seed=1)


def test_every_required_label_is_reached():
    assert KP.short(KP.runs()) == ([], [])


def test_removing_the_last_case_of_a_label_is_noticed():
    runs = KP.runs()
    L, P = KP.reached(runs)
    assert KP.REQUIRED <= L and KP.REQUIRED_PAIRS <= P
    for label in sorted(KP.REQUIRED):        # without the runs that reach it (in either form) the label is reported
        rest = [r for r in runs if label not in KP.labels_of_run(r, 0) | KP.labels_of_run(r, 1)]
        if label.startswith("form_"):
            continue                           # (every run has both forms: see below)
        assert label in KP.short(rest)[0], label
    for pair in sorted(KP.REQUIRED_PAIRS):
        rest = [r for r in runs if not (r["role"] == pair[0] and pair[1] in KP.labels_of_run(r, 0))]
        assert pair in KP.short(rest)[1], pair
    assert KP.short([])[0] == sorted(KP.REQUIRED)
    # the forms come from the GPU file's loop over convx_plan.PRODUCTS: both, for every run
    assert set(KP.XP_FORMS) == set(XP.PRODUCTS) == {0, 1}
    # labels that rest on one case name only: removing that case is reported
    for name, pair in (("wg_uneven", ("wgrad1", "wg_uneven")), ("wg_uneven_o", ("wgrad0", "wg_uneven"))):
        assert KP.short([r for r in runs if r["name"] != name]) == ([], [pair]), name
    assert KP.short([r for r in runs if not r["post"]]) == (["post"], [("dgrad1", "post_fold"), ("dgrad1", "post_inline")])


def test_gather_and_scatter_restatement_by_hand():
    W = np.arange(4 * 3 * 9, dtype=np.float32).reshape(4, 3, 3, 3)
    b = np.array([10, 11, 12, 13], np.float32)
    oidx = np.array([2, 0, -1, -1], np.int32)
    g = KP.gather_weights(W, oidx, 3, None, 3)
    assert np.array_equal(g[0], W[2]) and np.array_equal(g[1], W[0]) and not g[2].any()
    assert list(KP.gather_bias(b, oidx, 3)) == [12, 10, 0]
    cidx = np.array([1, -1, 2], np.int32)
    g = KP.gather_weights(W, None, 4, cidx, 2)
    assert np.array_equal(g[:, 0], W[:, 1]) and not g[:, 1].any() and g.shape == (4, 2, 3, 3)
    g = KP.gather_weights(W, oidx, 4, cidx, 3)
    assert np.array_equal(g[1, 2], W[0, 2]) and not g[2:].any() and not g[:, 1].any()
    # the scatter: the transpose of the gather -- <scatter(p), W> == <p, gather(W)> for every p
    rng = np.random.RandomState(0)
    p = rng.randn(4, 3, 3, 3)
    s = KP.scatter_add(np.zeros((4, 3, 3, 3)), p, oidx, cidx)
    assert np.isclose((s * W).sum(), (p * KP.gather_weights(W.astype(np.float64), oidx, 4, cidx, 3)).sum())
    assert not s[1].any() and not s[3].any() and not s[:, 0].any()          # filters / channels no entry names
    gw = np.full((4, 3, 3, 3), 7.0, np.float32)
    KP.scatter_add(gw, np.ones((4, 3, 3, 3)), oidx, cidx)
    assert (gw[2, 1] == 8).all() and (gw[0, 2] == 8).all() and (gw == 8).sum() == 4 * 9 and (gw[gw != 8] == 7).all()
    gb = KP.scatter_add_bias(np.zeros(4), np.array([1.0, 2.0, 3.0, 4.0]), oidx)
    assert list(gb) == [2, 0, 1, 0]


def test_planted_magnitudes():
    for c in KP.CASES:
        if not c["amax"] or not set(c["roles"]) & set(KP.CONV_ROLES):
            continue
        for role in KP.CONV_ROLES:
            d = KP.conv_inputs(dict(name=c["name"], role=role, post=False))
            part = d["w"][d["kept"]] if d["L"]["gather"] == "o" else d["w"][:, d["kept"]]
            ratio = float(np.abs(d["w"]).max() / np.abs(part).max())
            assert KP.amax_lies_in_kept(d["w"], d["kept"], d["L"]["gather"]) == (c["amax"] == "kept"), (c["name"], role)
            if c["amax"] == "dropped":          # ten binades, give or take the spread of the random weights
                assert KP.AMAX_FACTOR / 4 <= ratio <= KP.AMAX_FACTOR * 4, (c["name"], role, ratio)
            assert float(np.abs(d["wg"]).max()) == float(np.abs(part).max())


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16x6", "f16x3"])
def test_representation_share_with_the_full_tensors_magnitude(f16):
    """both splits emulated on the GATHERED operands, the weights scaled by the FULL tensor's largest magnitude (amax_b) as the
    gathered pack scales them: the kept plane products stay inside representation_bound taken with that magnitude.  Where the
    magnitude lies in a dropped filter 2^10 times larger than the kept ones (amax_in_dropped) the share that grows with it stays
    under the project's bar 1e-4 max(1, |result|): the rounding share of split_bound does not depend on the magnitude record, so
    the bar is as attainable for these inputs as for any other, and the GPU test holds the result to it."""
    worst = worst_bar = 0.0
    for r in KP.runs():
        if r["role"] not in KP.CONV_ROLES or r["post"]:
            continue
        d = KP.conv_inputs(r)
        full = float(np.abs(d["w"]).max())
        amax_a = float(np.abs(d["x"]).max())          # (fwd1: the raw tensor's; |slope| < 1)
        worst = max(worst, XP.representation_share(d["op"], d["act"], d["wg"], f16, KP.run_id(r), amax_a=amax_a, amax_b=full))
        rep = XP.representation_bound(d["op"], d["act"], d["wg"], f16, amax_a=amax_a, amax_b=full)
        bar = 1e-4 * np.maximum(1.0, np.abs(d["want"]))
        if d["case"]["amax"] == "dropped":
            worst_bar = max(worst_bar, float((rep / bar).max()))
            assert np.all(rep <= bar), (KP.run_id(r), float((rep / bar).max()))
            if f16:   # ... and it does grow with the magnitude: the share with the gathered part's own is smaller
                own = XP.representation_bound(d["op"], d["act"], d["wg"], f16, amax_a=amax_a)
                assert np.all(own <= rep) and float(rep.max()) > float(own.max())
    print("largest distance / representation share %.3f; largest share / bar with a dropped filter 2^10 larger: %.4f" % (worst, worst_bar))
    assert worst > 0.01


def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_header_ctypes_table_and_build_agree():
    """include/frcnn_hip_compact.h is included by frcnn_hip.h, declares exactly _lib.COMPACT_SIGS with their argument counts,
    stays out of the Lua binding, and is a dependency of the build; frcnn_hip.h's own list (tests/test_abi.py) does not change"""
    from frcnn_amd import _lib
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_compact.h")).read()
    names = set(_lib.COMPACT_SIGS)
    assert len(names) == 3
    assert '#include "frcnn_hip_compact.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names and not names & set(_lib.exported_symbols())
    assert not names & (set(_lib.HARD_SIGS) | set(_lib.LOSS_SIGS) | set(_lib.BOX_SIGS) | set(_lib.CLASSBOX_SIGS) | set(_lib.EVAL_SIGS) |
                        set(_lib.HEADS_SIGS))
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in names:
        m = re.search(r"^int %s\(([^;]*)\);" % name, code, re.M)
        assert m and len(m.group(1).split(",")) == len(_lib.COMPACT_SIGS[name][0]), name
    assert "frcnn_hip_compact.h" in open(os.path.join(ROOT, "build_lib.sh")).read()
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    assert not any(n in lua for n in names)
    for word in ("DISTINCT", "FULL", "exactly +0", "Untouched", "Refused before anything is launched", "g.amax = j.amax"):
        assert word in hdr, word
