"""Host-side pieces of the detection path that need no GPU: the single-problem workspace sizes are those of a one-segment
batch launch (the single entry points ARE that launch), and DeviceTensor.segment computes the segment views the Detector used
to spell as byte offsets."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2000])
def test_nms_workspace_is_the_one_segment_batch_workspace(F, n):
    L = F._lib.load()
    assert L.frcnn_nms_workspace_bytes(n) == L.frcnn_nms_batch_workspace_bytes(1, n)
    assert L.frcnn_nms_workspace_bytes(n) >= 256 + 24 * n + 8 * n * ((n + 63) // 64)    # four work arrays, mask, diagonal


@pytest.mark.parametrize("sizes", [[(55, 98), (27, 48), (25, 46), (23, 44)], [(1, 1)] * 4], ids=["vgg_small", "1x1"])
def test_scan_workspace_is_the_one_slot_batch_workspace(F, sizes):
    L = F._lib.load()
    Hs = (C.c_int * 4)(*[h for h, w in sizes]); Ws = (C.c_int * 4)(*[w for h, w in sizes])
    anchors = 3 * sum(h * w for h, w in sizes)
    assert L.frcnn_rpn_scan_workspace_bytes(Hs, Ws) == L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, 1)
    assert L.frcnn_rpn_scan_workspace_bytes(Hs, Ws) >= 256 + 41 * anchors    # rect, p and flag of every anchor


BASE = 0x7f0000001000    # a made-up address: no view below touches memory


@pytest.mark.parametrize("shape,dtype,row_bytes", [((3, 7, 5), np.float32, 20), ((3, 7, 4), np.float64, 32), ((3, 7), np.int64, 8),
                                                   ((3, 7), np.int32, 4), ((4, 3), np.int32, 4)],
                         ids=["float32x5", "float64x4", "int64", "int32", "counts"])
def test_segment_views(F, shape, dtype, row_bytes):
    t = F.DeviceTensor(BASE, shape, dtype)
    B, S = shape[:2]
    for b in range(B):
        v = t.segment(b)
        assert v.ptr == BASE + row_bytes * b * S and v.shape == shape[1:] and v.dtype == np.dtype(dtype)
        for rows in (0, 1, S):
            v = t.segment(b, rows)
            assert v.ptr == BASE + row_bytes * b * S and v.shape == (rows,) + shape[2:] and v.dtype == np.dtype(dtype)
            assert v.nbytes == row_bytes * rows
    assert type(t.segment(1).ptr) is int


def test_segment_out_of_range(F):
    t = F.DeviceTensor(BASE, (3, 7, 5), np.float32)
    for b, rows in ((3, None), (-1, None), (0, 8), (0, -1)):
        with pytest.raises(IndexError):
            t.segment(b, rows)
