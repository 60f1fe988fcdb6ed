"""cfg["box_head"] without a device: the setting's acceptances and refusals, the parameter counts and the table of a per-class
model, the numpy restatement (tests/box_head_ref.py) against hand-computed 2-class cases, the entry points' argument errors
(returned before any launch), and the declarations for both hosts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import box_head_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the setting
def test_settings_accepted(F):
    st = F.box_head_settings
    for cfg in (dict(), dict(box_head={}), dict(box_head=dict(per_class=False)), dict(box_head=None),
                dict(box_head=dict(per_class=np.bool_(False)))):
        assert st(cfg) == dict(per_class=False)
    assert st(dict(box_head=dict(per_class=True))) == dict(per_class=True)
    assert st(dict(box_head=dict(per_class=True), scoring=dict(classes="top"))) == dict(per_class=True)
    assert st(dict(box_head=dict(per_class=False), scoring=dict(classes="all"))) == dict(per_class=False)


@pytest.mark.parametrize("bad,word", [
    (dict(box_head=dict(per_klass=True)), "unknown"), (dict(box_head=dict(per_class=True, rows=4)), "unknown"),
    (dict(box_head=dict(per_class=1)), "boolean"), (dict(box_head=dict(per_class="true")), "boolean"),
    (dict(box_head=dict(per_class=None)), "boolean"), (dict(box_head=dict(per_class=0.0)), "boolean"),
    (dict(box_head=True), "table"), (dict(box_head=[True]), "table"),
])
def test_settings_refused(F, bad, word):
    with pytest.raises(F.FrcnnError, match=word):
        F.box_head_settings(bad)


def test_all_class_scoring_is_refused_with_both_keys_named(F):
    cfg = dict(F.duplo_cfg, box_head=dict(per_class=True), scoring=dict(classes="all"))
    with pytest.raises(F.FrcnnError) as e:
        F.box_head_settings(cfg)
    assert "box_head.per_class" in str(e.value) and "scoring.classes" in str(e.value)
    with pytest.raises(F.FrcnnError):
        F.vgg_small(cfg)                                   # create_model validates before the library is called
    # a Detector given the setting later refuses it too, naming both keys
    from frcnn_amd.Detector import Detector
    d = Detector.__new__(Detector)
    d.model = F.vgg_small(dict(F.duplo_cfg, box_head=dict(per_class=True)))
    d.set_scoring(dict(classes="top"))
    with pytest.raises(F.FrcnnError) as e:
        d.set_scoring(dict(classes="all"))
    assert "box_head.per_class" in str(e.value) and "scoring.classes" in str(e.value) and d.scoring == ("top", 0.2, None)


# -------------------------------------------------------------------------------------------------------- counts and the table
def test_parameter_counts_and_table(F):
    base = F.vgg_small(dict(F.duplo_cfg))["native"]
    assert F.duplo_cfg["class_count"] == 16 and base.total_params == 26784106
    for bh in ({}, dict(per_class=False)):
        nat = F.vgg_small(dict(F.duplo_cfg, box_head=bh))["native"]
        assert (nat.total_params, nat.pnet_params) == (26784106, 12089683) and nat.desc.box_per_class == 0
        assert np.array_equal(nat.param_table, base.param_table)
    per = F.vgg_small(dict(F.duplo_cfg, box_head=dict(per_class=True)))["native"]
    nf, Cn = 512, 16
    grow = 4 * (Cn - 1) * (nf + 1)
    assert per.desc.box_per_class == 1 and per.total_params == base.total_params + grow and per.pnet_params == base.pnet_params
    tb, tp = base.param_table, per.param_table
    assert len(tb) == len(tp)
    iw = len(tb) - 4                                        # the box head's weight, bias, then the class head's two
    assert np.array_equal(tp[:iw], tb[:iw])
    assert tuple(tb[iw]) == (tb[iw][0], 4 * nf, 3, nf) and tuple(tb[iw + 1]) == (tb[iw][0] + 4 * nf, 4, 4, nf)
    assert tuple(tp[iw]) == (tb[iw][0], 4 * Cn * nf, 3, nf)                       # same place, kinds 3 and 4 as now
    assert tuple(tp[iw + 1]) == (tb[iw][0] + 4 * Cn * nf, 4 * Cn, 4, nf)
    for k in (iw + 2, iw + 3):                              # every offset behind the head moves by that amount
        assert tp[k][0] == tb[k][0] + grow and tuple(tp[k][1:]) == tuple(tb[k][1:])
    assert int(tp[-1][0] + tp[-1][1]) == per.total_params
    # init_parameters needs no change: the two tensors are drawn like any Linear's, within 1 / sqrt(fan_in)
    w = per.init_parameters(seed=1)
    blk = w[tp[iw][0]:tp[iw + 1][0] + tp[iw + 1][1]]
    assert blk.shape[0] == 4 * Cn * (nf + 1) and np.abs(blk).max() <= (1 + 1e-6) / np.sqrt(nf) and np.count_nonzero(blk) > 0.99 * blk.size
    # one class: the per-class layout IS the shared layout
    one = dict(F.duplo_cfg, class_count=1)
    a, b = F.vgg_small(dict(one))["native"], F.vgg_small(dict(one, box_head=dict(per_class=True)))["native"]
    assert a.total_params == b.total_params and np.array_equal(a.param_table, b.param_table) and b.desc.box_per_class == 1
    # imgnet_cfg: 200 classes on 512 features
    big = F.vgg_large(dict(F.imgnet_cfg, box_head=dict(per_class=True)))["native"]
    assert big.total_params == 38631013 + 4 * 199 * 513


def test_model_desc_field_is_the_last_one(F):
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} frcnn_model_desc;", hdr, re.S).group(1), flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-1] == "int box_per_class" and F._lib.ModelDesc._fields_[-1] == ("box_per_class", C.c_int)
    assert F._lib.ModelDesc._fields_[-2][0] == "kw"
    d = F._lib.ModelDesc()
    assert d.box_per_class == 0                             # a zero-initialised caller keeps today's model


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_first_maximum_rule():
    nan, inf = np.nan, np.inf
    for row, want in (([-1, -2, -3], 0), ([-3, -1, -1], 1), ([-2, -2, -2], 0), ([nan, 5, 6], 0), ([-3, nan, -1], 2),
                      ([-3, nan, -3], 0), ([-inf, -inf, -inf], 0), ([-inf, nan, -2], 2), ([-1, inf, inf], 1), ([nan], 0)):
        assert B.first_maximum(np.array(row, np.float32)) == want, row


def test_class_sources_by_hand():
    Cn = 2
    assert B.select(5, Cn, "int", [2, 1, 2, 1, 2], 3).tolist() == [2, 1, 2, 0, 0]
    assert B.select(3, Cn, "int", [2, 1, 2], 0).tolist() == [0, 0, 0]
    assert B.select(6, Cn, "int", [0, 3, -3, 10 ** 9, 1, 2], 6).tolist() == [0, 0, 0, 0, 1, 2]
    t = np.array([1, 2, 3, 0, -3, 1e9, np.nan, 2.5, 0.99, 1.5, np.inf], np.float32)
    assert B.select(len(t), Cn, "float", t).tolist() == [1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    lsm = np.array([[-1, -2, -3], [-2, -1, -3], [-3, -2, -1], [-1, -1, -1], [np.nan, 0, 0], [-5, np.nan, -5]], np.float32)
    assert B.select(6, Cn, "argmax", lsm=lsm).tolist() == [1, 2, 0, 1, 1, 1]      # (row 2: the background is the maximum)


def test_kernels_by_hand():
    """two classes, two features: W rows 0..3 = class 1, rows 4..7 = class 2"""
    x = np.array([[1, 2], [3, -1], [0, 5], [2, 2]], np.float32)
    W = np.array([[1, 0], [0, 1], [1, 1], [2, -1], [10, 0], [0, 10], [10, 10], [-10, 10]], np.float32)
    b = np.array([0.5, 0, 0, 0, 100, 0, 0, 0], np.float32)
    sel = np.array([1, 2, 0, 2], np.int32)
    out, mag = B.forward(x, W, b, sel)
    assert out.tolist() == [[1.5, 2, 3, 0], [130, -10, 20, -40], [0, 0, 0, 0], [120, 20, 40, 0]]
    assert mag[1].tolist() == [130, 10, 40, 40] and not mag[2].any()
    g = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [7, 7, 7, 7], [1, 1, 1, 1]], np.float32)
    gf, gmag = B.input_gradient(g, W, sel)
    assert gf.tolist() == [[3, -1], [0, 10], [0, 0], [10, 30]] and gmag[3].tolist() == [30, 30]
    wg = B.weight_gradient(g, x, sel, 2, np.ones_like(W), np.ones_like(b))
    assert wg["gW"][:4].tolist() == [[2, 3], [1, 1], [1, 1], [2, 3]]            # class 1: row 0 alone, on a prior of ones
    assert wg["gW"][4:].tolist() == [[3, 3], [6, 2], [3, 3], [3, 3]]            # class 2: rows 1 and 3
    assert wg["gb"].tolist() == [2, 1, 1, 2, 2, 3, 2, 2] and wg["n"].tolist() == [1, 2] and wg["touched"].all()
    none = B.weight_gradient(g, x, np.array([1, 1, 0, 1]), 2, np.ones_like(W), np.ones_like(b))
    assert none["touched"].tolist() == [True, False] and np.array_equal(none["gW"][4:], np.ones((4, 2)))
    assert B.forward_bound(2, mag)[0, 0] == 4 * 2.0 ** -24 * 1.5


# ------------------------------------------------------------------------------------------------------ the entry points' errors
def test_argument_errors_are_returned_before_any_launch(F):
    """every refused call returns FRCNN_ERR_ARG with a message; the pointers are never dereferenced (they are not device memory
    here), and R <= 0 launches nothing"""
    lib = F._lib.load()
    p = C.c_void_p(0x1000)       # 16-byte aligned, never read
    odd = C.c_void_p(0x1002)

    def fwd(x=p, R=8, nf=16, W=p, b=p, Cn=2, cls=p, kind=1, n=4, lsm=None, ncls=0, out=p, sel=p):
        return lib.frcnn_box_head_forward(x, R, nf, W, b, Cn, cls, kind, n, lsm, ncls, out, sel, None)

    def bwd(g=p, x=p, sel=p, R=8, nf=16, W=p, Cn=2, gfeat=p, gW=p, gb=p):
        return lib.frcnn_box_head_backward(g, x, sel, R, nf, W, Cn, gfeat, gW, gb, None)

    bad_f = [dict(nf=0), dict(Cn=0), dict(kind=3), dict(kind=-1), dict(x=None), dict(W=None), dict(b=None), dict(out=None),
             dict(sel=None), dict(cls=None), dict(kind=2, cls=None), dict(n=-1), dict(n=9), dict(kind=0, cls=None),
             dict(kind=0, cls=None, lsm=p, ncls=0), dict(x=odd), dict(out=odd), dict(Cn=1 << 20, nf=1 << 10)]
    for kw in bad_f:
        assert fwd(**kw) != 0, kw
        assert lib.frcnn_last_error().decode().startswith("box_head_forward"), kw
    bad_b = [dict(nf=0), dict(Cn=0), dict(gW=None), dict(gb=None), dict(gfeat=None, gW=None, gb=None), dict(g=None), dict(sel=None),
             dict(W=None), dict(x=None), dict(gfeat=odd), dict(Cn=1 << 20, nf=1 << 10)]
    for kw in bad_b:
        assert bwd(**kw) != 0, kw
        assert lib.frcnn_last_error().decode().startswith("box_head_backward"), kw
    # nothing to do: no launch, no error -- also with every array NULL
    for R in (0, -5):
        assert fwd(R=R) == 0 and bwd(R=R) == 0
        assert fwd(R=R, x=None, W=None, b=None, cls=None, out=None, sel=None) == 0
    with pytest.raises(F.FrcnnError, match="classes"):
        F._lib.call("frcnn_box_head_forward", p, 8, 16, p, p, 2, None, 1, 4, None, 0, p, p, None)


def test_class_source_entry_point_needs_a_per_class_model(F):
    shared = F.vgg_small(dict(F.duplo_cfg))
    per = F.vgg_small(dict(F.duplo_cfg, box_head=dict(per_class=True)))
    p = C.c_void_p(0x1000)
    with pytest.raises(F.FrcnnError, match="shared"):
        F._lib.call("frcnn_cnet_box_classes", shared["native"].h, p, 1, 4)
    with pytest.raises(F.FrcnnError, match="shared"):
        shared["cnet"]._box_classes(("int", 0x1000, 4), 8)
    for args in ((p, 3, 0), (None, 1, 4), (None, 2, 0), (p, 1, -1)):
        with pytest.raises(F.FrcnnError, match="cnet_box_classes"):
            F._lib.call("frcnn_cnet_box_classes", per["native"].h, *args)
    for args in ((p, 1, 4), (p, 2, 0), (None, 0, 0)):
        F._lib.call("frcnn_cnet_box_classes", per["native"].h, *args)
    for bad in (("int", 0x1000), ("float", 0x1000, 3), ("long", 0x1000, 3)):
        with pytest.raises(F.FrcnnError, match="box_classes"):
            per["cnet"]._box_classes(bad, 8)
    with pytest.raises(F.FrcnnError, match="foreground rows"):
        per["cnet"]._box_classes(("int", 0x1000, 9), 8)


# ------------------------------------------------------------------------------------------------------------ the declarations
def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_are_declared_for_both_hosts(F):
    """the three entry points live in include/frcnn_hip_box.h, which frcnn_hip.h includes: the library exports them, the host
    mirror's fourth ctypes table and the Lua binding's fourth generated cdef declare exactly them with the header's argument
    counts, and the Lua files call them through the CB handle only"""
    names = {"frcnn_box_head_forward", "frcnn_box_head_backward", "frcnn_cnet_box_classes"}
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_box.h")).read()
    assert '#include "frcnn_hip_box.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names == set(F._lib.BOX_SIGS)
    assert not names & (set(F._lib.exported_symbols()) | set(F._lib.HARD_SIGS) | set(F._lib.LOSS_SIGS))
    for name, nargs in (("frcnn_box_head_forward", 14), ("frcnn_box_head_backward", 11), ("frcnn_cnet_box_classes", 4)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m and len(m.group(1).split(",")) == len(F._lib.BOX_SIGS[name][0]) == nargs, name
    lib = C.CDLL(F._lib.SO_PATH)
    assert all(hasattr(lib, n) for n in names) and all(getattr(F._lib.load(), n).argtypes for n in names)
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    fourth = re.findall(r"ffi\.cdef\(\[\[(.*?)\]\]\)", lua, re.S)
    assert len(fourth) == 1 and _symbols(fourth[0]) == names
    first = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert "int box_per_class;" in first and not names & _symbols(first)
    used = set()
    for fn in ("frcnn_hip.lua", "objective_hip.lua", "Detector_hip.lua", "frcnn_shims.lua.in"):
        txt = open(os.path.join(ROOT, "bindings", fn)).read()
        used |= set(re.findall(r"\bCB\.(frcnn_[a-z0-9_]+)", txt))
        for n in names:
            assert not re.search(r"\bC[HL]?\.%s\b" % n, txt), (fn, n)
    assert used == {"frcnn_cnet_box_classes"}
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    obj = open(os.path.join(ROOT, "bindings", "objective_hip.lua")).read()
    det = open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read()
    assert "function M.box_head_settings(cfg)" in shim and "d.box_per_class = box_head.per_class and 1 or 0" in shim
    assert obj.count("model.box_per_class and") == 3 and "box_head.per_class" in det
    for name in ("box_head", "box_head_settings"):
        assert name in F.__all__ and callable(getattr(F, name))
    assert "box_head.hip" in open(os.path.join(ROOT, "build_lib.sh")).read()
