"""The gradient guard without a device: configuration errors raised before any device call, the header / ctypes table / Lua
binding agreeing on the new entry points, and the Lua drop-in's dispatch (static text checks: no Lua runtime here)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("frcnn_grad_clip_workspace_bytes", "frcnn_grad_clip", "frcnn_scale_rmsprop_slice_dev", "frcnn_sgd_slice_dev",
       "frcnn_nag_slice_dev")


class _Untouchable(object):
    """stands for the weights: any use of it (a device pointer, its size, a copy) fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the weights were touched (%s) before the configuration was checked" % name)


@pytest.mark.parametrize("fn", ["rmsprop", "sgd", "nag"])
@pytest.mark.parametrize("extra,exc", [
    (dict(clipNorm=float("nan")), ValueError),
    (dict(clipNorm=-0.5), ValueError),
    (dict(clipNorm=float("inf")), ValueError),
    (dict(clipNorm="1"), ValueError),
    (dict(clipNorm=[1.0]), ValueError),
    (dict(clipNorm=True), ValueError),
    (dict(skipNonFinite=1), ValueError),
    (dict(clipNorm=1.0, skipNonFinite="no"), ValueError),
    (dict(clipNorm=1.0, eager=True), "FrcnnError"),
    (dict(skipNonFinite=True, eager=True), "FrcnnError"),
])
def test_guard_configuration_errors_come_before_any_device_call(F, fn, extra, exc):
    def opfunc(x):
        raise AssertionError("opfunc called")
    cfg = dict(extra)
    with pytest.raises(F.FrcnnError if exc == "FrcnnError" else exc) as e:
        getattr(F, fn)(opfunc, _Untouchable(), cfg)
    assert "clipNorm" in str(e.value) or "skipNonFinite" in str(e.value)
    assert cfg == extra, "the state was changed by a rejected call"


def test_guard_off_values_are_accepted(F):
    """None / 0 / False leave the guard off; a clipNorm implies skipNonFinite"""
    from frcnn_amd import utilities
    for cfg in (dict(), dict(clipNorm=None), dict(clipNorm=0), dict(clipNorm=0.0, skipNonFinite=False), dict(skipNonFinite=None)):
        assert utilities._guard_config(cfg, cfg, "sgd") is None
    assert utilities._guard_config(dict(clipNorm=2), {}, "sgd") == 2.0
    assert utilities._guard_config(dict(skipNonFinite=True), {}, "sgd") == 0.0
    assert utilities._guard_config(dict(clipNorm=0.5, skipNonFinite=False), {}, "sgd") == 0.5   # implied by clipNorm


def _header():
    src = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_ctypes_table_and_lua_binding_agree(F):
    raw, code = _header()
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    lib = C.CDLL(F._lib.SO_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), "%s missing from the header" % name
        assert name in F._lib.exported_symbols(), "%s missing from the ctypes table" % name
        assert re.search(r"\b%s\(" % name, cdef), "%s missing from the Lua cdef" % name
        assert hasattr(lib, name), "%s not exported by the library" % name
    # argument counts of the ctypes table against the header's declarations
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(F._lib._SIGS[name][0]), name
    assert F._lib._SIGS["frcnn_grad_clip_workspace_bytes"][1] is C.c_size_t
    # the semantics are defined once, in the header
    for word in ("S     =", "norm  =", "D'    =", "skipped", "record_dev: double[4]"):
        assert word in raw, word
    # host-only entry point: the workspace holds one fp64 partial per block of a grid sized from n alone
    wb = F._lib.load().frcnn_grad_clip_workspace_bytes
    assert wb(0) == 8 and wb(1) == 8 and wb(1024) == 8 and wb(2048) == 16 and wb(26_784_106) == 2048 * 8 == wb(1 << 40)


def test_lua_shims_honour_the_guard_keys():
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    assert shim in lua, "bindings/frcnn_hip.lua is not regenerated"
    assert "config.clipNorm" in shim and "config.skipNonFinite" in shim
    assert "C.frcnn_grad_clip(" in shim and "C.frcnn_grad_clip_workspace_bytes(" in shim
    for fn, calls in (("rmsprop", ("frcnn_scale_rmsprop_dev", "frcnn_scale_rmsprop_slice_dev")),
                      ("sgd", ("frcnn_sgd_slice_dev", "frcnn_sgd(")), ("nag", ("frcnn_nag_slice_dev", "frcnn_nag("))):
        m = re.search(r"\nfunction M\.%s\(.*?\n(.*?)\nend\n" % fn, shim, re.S)
        assert m, fn
        body = m.group(1)
        assert "guard_config(" in body and "guard_queue(x, dfdx, ranges, clip)" in body and "guard_report(x, record)" in body, fn
        for c in calls:
            assert "C." + c in body, (fn, c)
        assert body.index("guard_config(") < body.index("(x)"), "%s: the guard's settings are checked before opfunc runs" % fn
    assert "table.insert(stats.gnorm" in shim and "stats.skipped" in shim
    obj = open(os.path.join(ROOT, "bindings", "objective_hip.lua")).read()
    assert "stats = stats" in obj    # the objective publishes its stats table to the optim overrides


def test_docs_describe_the_guard():
    for fn, words in (("INTEGRATION.md", ("clipNorm", "skipNonFinite", "evalCounter", "gnorm")), ("README.md", ("clipNorm",)),
                      ("DESIGN.md", ("grad_sumsq_kernel",)), ("EXPERIMENTS.md", ("gradient guard",))):
        txt = open(os.path.join(ROOT, fn)).read()
        for w in words:
            assert w in txt, (fn, w)
