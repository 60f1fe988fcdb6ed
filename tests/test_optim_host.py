"""optim.sgd / optim.nag without a device: the -opti table (main.lua:35), configuration errors raised before anything is queued,
and the Lua drop-in's binding and dispatch (static text checks: no Lua runtime here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optimizer_maps_main_lua_opti_values(F):
    assert F.optimizer("rmsprop") is F.rmsprop
    assert F.optimizer("sgd") is F.sgd
    assert F.optimizer("nag") is F.nag
    for name in ("sgd", "nag", "optimizer"):
        assert name in F.__all__
    with pytest.raises(ValueError):
        F.optimizer("adam")


class _Untouchable(object):
    """stands for the weights: any use of it (a device pointer, its size, a copy) fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the weights were touched (%s) before the configuration was checked" % name)


@pytest.mark.parametrize("fn,cfg", [
    ("sgd", dict(momentum=0.9, nesterov=True)),                   # dampening defaults to momentum
    ("sgd", dict(momentum=0, dampening=0, nesterov=True)),
    ("sgd", dict(momentum=0.9, dampening=0.1, nesterov=True)),
    ("sgd", dict(learningRates=[1.0])),
    ("sgd", dict(weightDecays=[1.0])),
    ("nag", dict(momentum=0)),
    ("nag", dict(momentum=-0.9)),
    ("nag", dict(learningRates=[1.0])),
])
def test_configuration_errors_come_before_any_device_call(F, fn, cfg):
    def opfunc(x):
        raise AssertionError("opfunc called")
    with pytest.raises(ValueError) as e:
        getattr(F, fn)(opfunc, _Untouchable(), cfg)
    if "learningRates" in cfg or "weightDecays" in cfg:
        assert "per-parameter" in str(e.value)
    assert "dfdx" not in cfg and "evalCounter" not in cfg


def test_lua_binding_declares_the_optimisers():
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for name in ("frcnn_sgd", "frcnn_sgd_slice", "frcnn_nag", "frcnn_nag_slice", "frcnn_nag_lookahead"):
        assert re.search(r"\bint %s\(" % name, cdef), name
    for name in ("frcnn_sgd", "frcnn_nag", "frcnn_nag_lookahead"):
        assert "C.%s(" % name in lua, name


def test_lua_shims_install_sgd_and_nag_dispatch():
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    assert "function M.sgd(opfunc, x, config, state)" in shim and "function M.nag(opfunc, x, config, state)" in shim
    for name in ("sgd", "nag"):
        # device tensor -> the library, anything else -> Torch's own function
        m = re.search(r"optim\.%s = function\(opfunc, x, config, state\)[^\n]*\n(.*?)\n    end" % name, shim, re.S)
        assert m, name
        body = m.group(1)
        assert "if M.is_tensor(x) then return M.%s(opfunc, x, config, state) end" % name in body
        assert "return ref_%s(opfunc, x, config, state)" % name in body
    assert "local ref_sgd, ref_nag = optim.sgd, optim.nag" in shim
    # the state lives where optim keeps it: state.dfdx made by M.tensor, state.evalCounter in the table
    assert "state.dfdx = M.tensor({ x.n })" in shim and "state.evalCounter = state.evalCounter + 1" in shim
