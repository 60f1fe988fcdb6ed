"""The classification net and the operator entry points run ONE Linear (csrc/linear.h): layer 0 of a model, Linear(1152 -> 512)
without a batch normalisation, gives bit for bit what frcnn_linear_forward gives on the same input, weight slice and bias -- in
the fp32 form, in the three-plane form and in the two-plane fp16 form, at the smallest row count the split form takes
(1696 x 1152 x 512 = 1 000 341 504 >= 1e9) and one row below it.  Evaluate mode, FRCNN_CNET_FUSE=0 (the product folds its own
slabs into the buffer frcnn_model_debug_buffer shows).  Both fold their slabs in split order, so equality is exact.

tests/test_gpu_gemm_plans.py tests the entry points plan by plan; this file is what ties those tests to the model."""
import numpy as np
import pytest

import cnet_plan as CP
import decisions
from test_gpu_cnet_shapes import _Nets, _restore, layout
from test_gpu_convx_plans import _option

pytestmark = pytest.mark.gpu

KEY = ("bn_last", 32, CP.CLASS_COUNT)
I, O_ = CP.ROI_CELLS * 32, CP.TABLES["bn_last"][0][0]
SPLIT_ROWS = 1696
assert (I, O_) == (1152, 512) and not CP.TABLES["bn_last"][0][1]
assert (SPLIT_ROWS - 1) * I * O_ < 1e9 <= SPLIT_ROWS * I * O_


@pytest.fixture(scope="module")
def nets(F, O):
    return _Nets(F, O)


@pytest.fixture
def options(F):
    """-> set(name, value); x3_f16 is put back after the test, gemm_x_roles goes back to the built-in rule"""
    before = _option(F, "x3_f16")
    yield lambda name, value: _option(F, name, value)
    _option(F, "x3_f16", before)
    _option(F, "gemm_x_roles", -1)


_X = {}


def _x(R):
    if R not in _X:
        _X[R] = np.random.RandomState(R).randn(R, I).astype(np.float32)
        _X[R].setflags(write=False)
    return _X[R]


def _both(F, s, R):
    """-> (layer 0's Linear output of an evaluate-mode frcnn_cnet_forward, frcnn_linear_forward on the same operands)"""
    cnet, nat = s["model"]["cnet"], s["model"]["native"]
    d = layout(KEY, nat.pnet_params)[0][0]
    x = F.DeviceTensor.from_numpy(_x(R))
    try:
        cnet.evaluate()
        cnet.drop_masks = None
        cnet.forward(x)
        model = decisions._dev_array(F, nat, 3, 0, np.float32, (R, O_)).copy()
    finally:
        _restore(s)
    y = F.DeviceTensor.from_numpy(np.full((R, O_), np.nan, np.float32))
    base = s["weights"].data_ptr()
    F._lib.call("frcnn_linear_forward", F.ptr(x), R, I, F.ptr(base + 4 * d["W"]), F.ptr(base + 4 * d["b"]), O_, F.ptr(y), F.stream_ptr())
    return model, y.numpy().copy()


@pytest.mark.parametrize("R,roles,f16,split", [(SPLIT_ROWS, 7, 0, True), (SPLIT_ROWS, 7, 1, True), (SPLIT_ROWS, 0, 1, False),
                                               (SPLIT_ROWS - 1, 7, 1, False)],
                         ids=["three_plane", "fp16", "roles_off", "below_the_floor"])
def test_layer_0_is_the_entry_point_bit_for_bit(F, nets, options, monkeypatch, R, roles, f16, split):
    monkeypatch.setenv("FRCNN_CNET_FUSE", "0")
    s = nets.get(KEY)
    options("gemm_x_roles", 0)
    options("x3_f16", f16)
    fp32_model, fp32_entry = _both(F, s, R)
    assert np.isfinite(fp32_entry).all() and np.array_equal(fp32_model, fp32_entry), "fp32"
    options("gemm_x_roles", roles)
    model, entry = _both(F, s, R)
    assert np.isfinite(entry).all()
    assert np.array_equal(model, entry), "largest difference %.3e" % np.abs(model - entry).max()
    # the form the case is here for was the one taken, on both sides
    assert np.array_equal(entry, fp32_entry) != split and np.array_equal(model, fp32_model) != split
