"""optim.adam without a device: configuration errors raised before anything is touched, the host scalars of the restatement,
the three entry points' signatures in the header, the ctypes table and the generated Lua cdef, and the Lua drop-in's function
and dispatch (static text checks: no Lua runtime here)."""
import ctypes as C
import math
import os
import re

import pytest

from adam_ref import adam_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Untouchable(object):
    """stands for the weights: any use of it (a device pointer, its size, a copy) fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the weights were touched (%s) before the configuration was checked" % name)


@pytest.mark.parametrize("cfg", [
    dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=float("nan")),
    dict(beta2=1.0), dict(beta2=1.5), dict(beta2=-1e-3),
    dict(epsilon=0), dict(epsilon=-1e-8),
    dict(learningRate=-1e-3),
    dict(weightDecay=-5e-4),
    dict(weightDecay=5e-4, decoupled=1), dict(decoupled="yes"),
    dict(learningRates=[1.0]), dict(weightDecays=[1.0]),
    dict(clipNorm=-1.0), dict(clipNorm="big"), dict(skipNonFinite=1),
])
@pytest.mark.parametrize("separate_state", [False, True])
def test_configuration_errors_come_before_any_device_call(F, cfg, separate_state):
    def opfunc(x):
        raise AssertionError("opfunc called")
    cfg = dict(cfg)
    state = {} if separate_state else cfg
    with pytest.raises(ValueError) as e:
        if separate_state:
            F.adam(opfunc, _Untouchable(), cfg, state)
        else:
            F.adam(opfunc, _Untouchable(), cfg)
    if "learningRates" in cfg or "weightDecays" in cfg:
        assert "per-parameter" in str(e.value)
    for table in (cfg, state):
        assert "t" not in table and "m" not in table and "v" not in table


def test_guard_with_the_eager_update_is_refused_as_for_sgd(F):
    def opfunc(x):
        raise AssertionError("opfunc called")
    cfg = dict(clipNorm=1.0, eager=True)
    with pytest.raises(F.FrcnnError):
        F.adam(opfunc, _Untouchable(), cfg)
    assert "t" not in cfg and "m" not in cfg and "v" not in cfg


def test_adam_is_exported_and_optimizer_stays_main_luas_table(F):
    assert "adam" in F.__all__ and callable(F.adam)
    with pytest.raises(ValueError):
        F.optimizer("adam")
    assert "F.adam" in F.optimizer.__doc__


def test_adam_scalars_against_hand_computed_values():
    s1 = adam_scalars({}, 0)                                    # the first step: t = 1
    assert s1["step"] == 1e-3 * math.sqrt(1 - 0.999) / (1 - 0.9)
    assert s1["step"] == pytest.approx(3.1622776601683e-4, rel=1e-9)      # 1e-3 * sqrt(1e-3) / 0.1
    assert (s1["beta1"], s1["beta2"], s1["eps"], s1["wd"], s1["decay"]) == (0.9, 0.999, 1e-8, 0.0, 0.0)
    assert s1["omb1"] == 1 - 0.9 and s1["omb2"] == 1 - 0.999
    s2 = adam_scalars({}, 1)                                    # t = 2: 1 - 0.81 = 0.19, 1 - 0.998001 = 0.001999
    assert s2["step"] == 1e-3 * math.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    assert s2["step"] == pytest.approx(1e-3 * math.sqrt(0.001999) / 0.19, rel=1e-12)
    assert s2["step"] == pytest.approx(2.3531684e-4, rel=1e-6)
    # learningRateDecay uses the t from before the increment; decoupled decay is clr * weightDecay and leaves wd at 0
    s = adam_scalars(dict(learningRate=1e-2, learningRateDecay=0.25, weightDecay=5e-4, decoupled=True), 2)
    clr = 1e-2 / (1 + 2 * 0.25)
    assert s["decay"] == clr * 5e-4 and s["wd"] == 0.0
    assert s["step"] == clr * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
    s = adam_scalars(dict(weightDecay=5e-4), 0)
    assert s["wd"] == 5e-4 and s["decay"] == 0.0
    assert adam_scalars(dict(beta1=0), 5)["step"] == 1e-3 * math.sqrt(1 - 0.999 ** 6)


# the three signatures as the issue states them: parameter types in order
_TAIL = ["float"] * 8 + ["void *"]
SIGNATURES = {
    "frcnn_adam": ["float *"] * 4 + ["long long", "float", "const double *"] + _TAIL,
    "frcnn_adam_slice": ["float *"] * 4 + ["long long", "long long", "float"] + _TAIL,
    "frcnn_adam_slice_dev": ["float *"] * 4 + ["long long", "long long", "const double *"] + _TAIL,
}
_CTYPE = {"float *": C.c_void_p, "const double *": C.c_void_p, "void *": C.c_void_p, "long long": C.c_longlong, "float": C.c_float}


def _declared(text, name):
    m = re.search(r"\bint %s\(([^)]*)\);" % name, text)
    assert m, "%s is not declared" % name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        t = re.sub(r"\w+$", "", p).strip()                      # drop the parameter's name
        out.append(t)
    return out


def test_header_ctypes_table_and_lua_cdef_agree_on_the_signatures(F):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for name, want in SIGNATURES.items():
        assert _declared(hdr, name) == want, name
        assert _declared(cdef, name) == want, name
        argtypes, restype = F._lib._SIGS[name]
        assert restype is C.c_int and list(argtypes) == [_CTYPE[t] for t in want], name
        assert name in F._lib.exported_symbols()


def test_lua_shims_install_adam_and_its_dispatch():
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    assert "function M.adam(opfunc, x, config, state)" in shim
    body = shim[shim.index("function M.adam(opfunc, x, config, state)"):]
    body = body[:body.index("\nend\n")]
    for call in ("C.frcnn_adam(", "C.frcnn_adam_slice(", "C.frcnn_adam_slice_dev(", "guard_config(config, 'adam')",
                 "no_per_parameter(config, 'adam')", "guard_queue(", "guard_report(", "pass_ranges(x)"):
        assert call in body, call
    assert "state.m = state.m or M.tensor({ x.n }):zero()" in body and "state.v = state.v or M.tensor({ x.n }):zero()" in body
    assert "state.t = state.t + 1" in body and "config.decoupled" in body
    # device tensor -> the library, anything else -> Torch's own function
    m = re.search(r"optim\.adam = function\(opfunc, x, config, state\)[^\n]*\n(.*?)\n    end", shim, re.S)
    assert m
    assert "if M.is_tensor(x) then return M.adam(opfunc, x, config, state) end" in m.group(1)
    assert "return ref_adam(opfunc, x, config, state)" in m.group(1)
    assert "local ref_adam = optim.adam" in shim


def test_integration_guide_covers_adam():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "optim.adam" in doc and "decoupled" in doc and "AdamW" in doc
    para = [p for p in doc.split("\n\n") if "adam" in p.lower() and "skip" in p.lower()]
    assert para, "INTEGRATION.md does not say what a skipped step does to Adam"
    assert any("moments" in p for p in para)
    assert 'optimizer("adam")' in doc or "optimizer('adam')" in doc
