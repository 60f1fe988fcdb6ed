"""cfg.cnet_loss without a GPU: the setting is accepted and refused as documented, the numpy restatement the device tests compare
against (tests/cnet_loss_ref.py) has the gradients autograd gives and reduces to the reference's losses at its defaults, and
the entry point is declared for both hosts."""
import math
import os
import re

import numpy as np
import pytest

import anchor_ops_ref as A
import cnet_loss_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- settings
def test_defaults_and_absent(F):
    assert F.cnet_loss_settings({}) is None and F.cnet_loss_settings(dict(cnet_loss=None)) is None
    st = F.cnet_loss_settings(dict(cnet_loss={}))
    assert st == dict(cls="nll", gamma=2.0, alpha=None, label_smoothing=0.0, box="smooth_l1", beta=1.0, box_weight=10.0)
    assert st == L.DEFAULT
    st = F.cnet_loss_settings(dict(cnet_loss=dict(cls="focal", gamma=0, alpha=0.25, box="giou", beta=1.0 / 9, box_weight=0)))
    assert (st["cls"], st["gamma"], st["alpha"], st["box"], st["beta"], st["box_weight"]) == ("focal", 0.0, 0.25, "giou", 1.0 / 9, 0.0)
    assert F.cnet_loss_settings(dict(cnet_loss=dict(cls="focal", label_smoothing=0)))["label_smoothing"] == 0.0
    assert F.cnet_loss_settings(dict(cnet_loss=dict(label_smoothing=0.999, gamma=5)))["label_smoothing"] == 0.999
    from frcnn_amd.objective import cnet_loss_desc
    d = cnet_loss_desc(F.cnet_loss_settings(dict(cnet_loss=dict(box="giou"))), 21)
    assert (d.cls, d.box, d.bgclass, d.gamma, d.alpha, d.smoothing, d.beta, d.box_weight) == (0, 1, 21, 2.0, -1.0, 0.0, 1.0, 10.0)


BAD = [dict(cls="ce"), dict(cls=1), dict(box="iou"), dict(box=None), dict(gamma=-0.1), dict(gamma=5.5), dict(gamma=float("nan")),
       dict(gamma="2"), dict(gamma=True), dict(alpha=0), dict(alpha=1), dict(alpha=1.5), dict(alpha=-1), dict(alpha="0.25"),
       dict(alpha=float("inf")), dict(label_smoothing=1), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")),
       dict(cls="focal", label_smoothing=0.1), dict(beta=0), dict(beta=-1), dict(beta=float("inf")), dict(beta=None),
       dict(box_weight=-1), dict(box_weight=float("inf")), dict(box_weight=float("nan")), dict(box_weight=False),
       dict(smoothing=0.1), dict(focal=True)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join("%s=%r" % kv for kv in sorted(b.items())))
def test_refusals(F, bad):
    with pytest.raises(F.FrcnnError, match="cnet_loss"):
        F.cnet_loss_settings(dict(cnet_loss=bad))


def test_not_a_table_is_refused(F):
    for v in ("focal", 1, ["focal"], True):
        with pytest.raises(F.FrcnnError, match="cnet_loss"):
            F.cnet_loss_settings(dict(cnet_loss=v))


# ------------------------------------------------------------------------------------------------------ the restatement itself
def _torch_losses(c, d, ncls):
    """the same losses written with torch operations in float64 -> (sum of cls_r / R, sum of box_weight * box_r, leaves)"""
    import torch
    R, npos = c["R"], c["npos"]
    cc = torch.tensor(c["ccout"].astype(np.float64), requires_grad=True)
    cr = torch.tensor(c["crout"].astype(np.float64), requires_grad=True)
    ct = torch.tensor(c["crtarget"].astype(np.float64))
    t = torch.tensor(c["cctarget"].astype(np.int64) - 1)
    w = torch.ones(R, dtype=torch.float64)
    if d["alpha"] is not None:
        w = torch.where(t + 1 == ncls, torch.tensor(1.0 - d["alpha"], dtype=torch.float64), torch.tensor(d["alpha"], dtype=torch.float64))
    lp = cc[torch.arange(R), t]
    if d["cls"] == "focal" and d["gamma"] > 0:
        cls = -w * (1.0 - torch.exp(lp)) ** d["gamma"] * lp
    elif d["label_smoothing"] > 0:
        e = d["label_smoothing"]
        cls = -w * ((1.0 - e) * lp + e / ncls * cc.sum(1))
    else:
        cls = -w * lp
    fgm = (torch.arange(R) < npos).to(torch.float64)[:, None]
    v = cr * fgm
    if d["box"] == "smooth_l1":
        z = v - ct
        # (the kernel takes the difference in fp32: its rounding, a constant of the row, is added so that the values agree too)
        z32 = ((c["crout"] * fgm.numpy().astype(np.float32)) - c["crtarget"]).astype(np.float32).astype(np.float64)
        z = z + (torch.tensor(z32) - z.detach())
        b = d["beta"]
        box = torch.where(z.abs() < b, 0.5 * z * z / b, z.abs() - 0.5 * b).sum(1)
    else:
        x0, y0 = cr[:, 0], cr[:, 1]
        x1, y1 = x0 + torch.exp(torch.clamp(cr[:, 2], max=L.K)), y0 + torch.exp(torch.clamp(cr[:, 3], max=L.K))
        tx0, ty0 = ct[:, 0], ct[:, 1]
        tx1, ty1 = tx0 + torch.exp(ct[:, 2]), ty0 + torch.exp(ct[:, 3])
        iw = (torch.min(x1, tx1) - torch.max(x0, tx0)).clamp(min=0)
        ih = (torch.min(y1, ty1) - torch.max(y0, ty0)).clamp(min=0)
        I = iw * ih
        U = (x1 - x0) * (y1 - y0) + (tx1 - tx0) * (ty1 - ty0) - I
        Cc = (torch.max(x1, tx1) - torch.min(x0, tx0)) * (torch.max(y1, ty1) - torch.min(y0, ty0))
        box = (2.0 - I / U - U / Cc) * fgm[:, 0]
    return (cls / R).sum(), (d["box_weight"] * box).sum(), cc, cr


@pytest.mark.parametrize("name", ["smoothed_alpha", "focal2", "focal_half", "focal1_giou", "beta_ninth", "giou", "nll_alpha"])
def test_gradients_against_autograd(name):
    """the four gradients (NLL / smoothed, focal, SmoothL1, GIoU) on rows away from ties: each stored float is the rounding of
    a double that agrees with autograd's to 1e-12 relative to the row's scale (both are float64 evaluations of one formula)"""
    d = dict(L.DESCS[name])
    if d["box_weight"] == 0.0:
        d["box_weight"] = 1.5
    c = L.random_rows(41, 70, 5, 30)
    ref = L.loss_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], d)
    lc, lb, cc, cr = _torch_losses(c, d, 5)
    (lc + lb).backward()
    gcc, gcr = cc.grad.numpy(), cr.grad.numpy()
    assert np.all(np.abs(ref["ccdelta"] - gcc) <= L.spacing32(ref["ccdelta"]) + 1e-12 * (1 + np.abs(gcc)))
    assert np.all(np.abs(ref["crdelta"][:30] - gcr[:30]) <= L.spacing32(ref["crdelta"][:30]) + 1e-12 * (1 + np.abs(gcr[:30])))
    assert np.any(gcc != 0) and np.any(gcr[:30] != 0)
    (s0, s1), _ = L.accumulate_ref(ref["row_loss"])
    lc, lb = lc.detach(), lb.detach()
    assert abs(s1 - float(lc)) <= 1e-12 * (1 + abs(float(lc))) and abs(s0 - float(lb)) <= 1e-12 * (1 + abs(float(lb)))
    if d["box"] == "giou":     # a background row has no box term
        assert not ref["crdelta"][30:].any() and not ref["box"][30:].any()
        assert ref["box"][:30].min() >= 0.0 and ref["box"][:30].max() <= 2.0


def test_default_desc_is_the_reference_loss():
    """at the defaults the restatement is anchor_ops_ref.cnet_losses_ref: crdelta, ccdelta and the zeroed crout bit for bit;
    the sums within one fp32 unit of the parent's fp32-rounded sums plus frcnn_loss_accumulate's bound"""
    for R in (1, 63, 65, 257):
        for ncls in (2, 17):
            for npos in A.cnet_npos(R):
                c = A.cnet_losses_case(R, npos, ncls)
                want = c["want"]
                got = L.loss_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], npos, L.DEFAULT)
                assert got["crdelta"].tobytes() == want["crdelta"].tobytes()
                assert got["ccdelta"].tobytes() == want["ccdelta"].tobytes()
                assert got["crout"].tobytes() == want["crout"].tobytes()
                (creg, ccls), (b0, b1) = L.accumulate_ref(got["row_loss"])
                # the parent rounds its exact sum to fp32 once (and scales the box sum by 10 behind that); a row's own term carries
                # at most 8 fp64 roundings
                own = 8 * 2.0 ** -53 * np.abs(got["row_loss"]).sum(0)
                assert abs(creg - float(np.float32(want["reg_sum"])) * 10.0) <= 10.0 * float(np.spacing(np.float32(abs(want["reg_sum"])))) + b0 + own[0]
                assert abs(ccls - float(np.float32(want["cls_mean"]))) <= float(np.spacing(np.float32(abs(want["cls_mean"])))) + b1 + own[1]


def test_gamma_zero_and_no_smoothing_are_nll():
    c, _, _ = L.case(65, 17, 1, "default")
    args = (c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"])
    base = L.loss_ref(*args, L.DEFAULT)
    for d in (L.desc(cls="focal", gamma=0.0), L.desc(label_smoothing=0.0), L.desc(cls="focal", gamma=0.0, label_smoothing=0.0)):
        got = L.loss_ref(*args, d)
        for k in ("ccdelta", "crdelta", "key", "row_loss", "crout"):
            assert got[k].tobytes() == base[k].tobytes(), k
    # ... and with alpha both carry the same weights
    a, b = L.loss_ref(*args, L.desc(alpha=0.3)), L.loss_ref(*args, L.desc(cls="focal", gamma=0.0, alpha=0.3))
    assert a["ccdelta"].tobytes() == b["ccdelta"].tobytes() and a["key"].tobytes() == b["key"].tobytes()


def test_special_values_of_the_restatement():
    c, lab, d = L.case(300, 21, 300, "focal1_giou")
    ref = L.loss_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], d, roi=c["roi"])
    for r in lab["bad_target"]:
        assert ref["key"][r] == -np.inf and np.isnan(ref["cls"][r]) and not ref["ccdelta"][r].any()
    for r in lab["nan_input"] + lab["neg_inf_target"]:
        assert ref["key"][r] == np.inf
    for r in lab["neg_inf_target"]:       # p log p -> 0: the gradient is -w q^g / R, not a NaN
        assert np.isfinite(ref["ccdelta"][r]).all() and ref["ccdelta"][r, int(c["cctarget"][r]) - 1] == np.float32(-1.0 / 300)
    for r in lab["p_t_one"]:
        assert ref["cls"][r] == 0 and not ref["ccdelta"][r].any()
    for r in lab["giou_equal"]:
        assert ref["box"][r] == 0.0 and not ref["crdelta"][r].any()
    for r in lab["giou_disjoint"]:
        assert ref["box"][r] > 1.0 and not ref["info"][r]["has"]
    for r in lab["giou_partial"]:
        assert 0.0 < ref["box"][r] < 1.0 and ref["info"][r]["has"] and not ref["info"][r]["inside"]
    for r in lab["giou_inside"]:
        assert ref["info"][r]["inside"]
    for r in lab["giou_edge_tie"]:
        assert ref["info"][r]["ties"][0] and ref["info"][r]["ties"][1]
    for r in lab["giou_above_K"]:
        assert ref["info"][r]["clamp"] == (True, True) and not ref["crdelta"][r, 2:].any() and ref["crdelta"][r, :2].any()
    assert ref["box5"][:, :4].tobytes() == c["roi"].astype(np.float32).tobytes() and ref["box5"][:, 4].tobytes() == ref["key"].tobytes()
    # |z| at beta: the quadratic branch below it, the linear one from it on
    c, lab, d = L.case(65, 17, 65, "beta_half")
    ref = L.loss_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], d)
    r = lab["z_at_beta"][0]
    assert ref["crdelta"][r, 0] < 1.0 and ref["crdelta"][r, 1] == 1.0 and ref["crdelta"][r, 2] == -1.0 and ref["crdelta"][r, 3] == -1.0


def test_every_label_is_reached_by_two_cases():
    seen = dict((k, 0) for k in L.LABELS)
    for (R, ncls, npos) in L.SHAPES:
        for name in L.DESCS:
            _, lab, _ = L.case(R, ncls, npos, name)
            for k, rows in lab.items():
                seen[k] += 1 if rows else 0
    assert all(v >= 2 for v in seen.values()), seen
    assert any((R * ncls) % 4 for R, ncls, _ in L.SHAPES)
    assert {R for R, _, _ in L.SHAPES} == {1, 63, 64, 65, 300} and {n for _, n, _ in L.SHAPES} == {2, 3, 17, 21}
    for R in (1, 63, 64, 65, 300):
        assert {p for r, _, p in L.SHAPES if r == R} >= ({0, 1, R} if R > 1 else {0, 1})


def test_accumulate_ref_is_a_sum():
    rng = np.random.RandomState(3)
    x = rng.randn(300, 2) * 10
    (a, b), (ba, bb) = L.accumulate_ref(x)
    assert abs(a - math.fsum(x[:, 0])) <= ba and abs(b - math.fsum(x[:, 1])) <= bb


# ------------------------------------------------------------------------------------------------------------ the declaration
def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_point_is_declared_for_both_hosts(F):
    """frcnn_cnet_loss_rows lives in include/frcnn_hip_loss.h, which frcnn_hip.h includes: the library exports it, the host
    mirror's third ctypes table and the Lua binding's third generated cdef declare exactly that, the structure has the header's
    fields, and the Lua files call it through the CL handle only."""
    import ctypes
    names = {"frcnn_cnet_loss_rows"}
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_loss.h")).read()
    assert '#include "frcnn_hip_loss.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names == set(F._lib.LOSS_SIGS)
    assert not names & set(F._lib.exported_symbols()) and not names & set(F._lib.HARD_SIGS)
    m = re.search(r"^int frcnn_cnet_loss_rows\(([^;]*)\);", hdr, re.M)
    assert m and len(m.group(1).split(",")) == len(F._lib.LOSS_SIGS["frcnn_cnet_loss_rows"][0]) == 15
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} frcnn_cnet_loss_desc;", hdr, re.S).group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            fields += [(n.strip(), ty) for n in rest.split(",")]
    ct = {"int": ctypes.c_int, "double": ctypes.c_double}
    assert [(n, ct[ty]) for n, ty in fields] == list(F._lib.CnetLossDesc._fields_)
    assert ctypes.sizeof(F._lib.CnetLossDesc) == 56
    lib = ctypes.CDLL(F._lib.SO_PATH)
    assert hasattr(lib, "frcnn_cnet_loss_rows") and F._lib.load().frcnn_cnet_loss_rows.argtypes
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdefs = re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, re.S)
    assert len(cdefs) == 3 and _symbols(cdefs[2]) == names and "frcnn_cnet_loss_desc;" in cdefs[2]
    assert not names & (_symbols(cdefs[0]) | _symbols(cdefs[1]))
    used = set()
    for fn in ("frcnn_hip.lua", "objective_hip.lua", "Detector_hip.lua", "frcnn_shims.lua.in"):
        txt = open(os.path.join(ROOT, "bindings", fn)).read()
        used |= set(re.findall(r"\bCL\.(frcnn_[a-z0-9_]+)", txt))
        assert not re.search(r"\bCH?\.frcnn_cnet_loss_rows", txt), fn
    assert used == names
    for name in ("cnet_loss", "cnet_loss_settings"):
        assert name in F.__all__ and callable(getattr(F, name))
