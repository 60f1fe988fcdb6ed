"""The greedy NMS scan (csrc/nms.hip nms_reduce_body) on problems built to reach each of its wave roles: the diagonal wave at
64 ballot rounds, every helper wave, the background waves' words in registers and their immediate loop, in the first and in a
second 64-word piece (tests/nms_plan.py builds the problems and labels them; tests/test_nms_plan.py checks the labels).
Every comparison is exact equality of the id lists, with the closed form and with the oracle."""
import ctypes as C

import numpy as np
import pytest

import nms_plan as NP

pytestmark = pytest.mark.gpu
SENTINEL = -7
S = NP.SCAN_CASE


def _padded(rows, n_cap, extra_cols=0):
    """rows in a buffer of n_cap rows, NaN behind them"""
    out = np.full((n_cap, rows.shape[1] + extra_cols), np.nan, np.float32)
    out[:len(rows), :rows.shape[1]] = rows
    return out


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))     # (NaN rows compare as bits)


def _device_n(F, rows, n_cap, thr, cls=None, key_mode=0, key_col=0):
    """frcnn_nms_device_n: the rows in a buffer of n_cap rows (NaN behind them), their count in device memory.  Returns the
    pick list; nothing may be stored behind it."""
    n = len(rows)
    buf = _padded(rows, n_cap)
    db = F.DeviceTensor.from_numpy(buf)
    dc = F.DeviceTensor.from_numpy(np.concatenate([cls, np.zeros(n_cap - n, np.int32)])) if cls is not None else None
    ndev = F.DeviceTensor.from_numpy(np.array([n], np.int32))
    wsb = F._lib.load().frcnn_nms_workspace_bytes(n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    pick = F.DeviceTensor.from_numpy(np.full(n_cap + 64, SENTINEL, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(2, SENTINEL, np.int32))
    F._lib.call("frcnn_nms_device_n", F.ptr(db), n_cap, F.ptr(ndev), buf.shape[1], C.c_float(thr), key_mode, key_col, F.ptr(dc),
                F.ptr(pick), F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
    k, host = cnt.numpy(), pick.numpy()
    assert 0 <= k[0] <= n and k[1] == SENTINEL
    assert np.all(host[k[0]:] == SENTINEL), "stores behind the %d picks" % k[0]
    assert _same_bytes(db.numpy(), buf)
    return host[:k[0]].tolist()


def _device_classes(F, rows, thr, cls):
    """frcnn_nms_device_classes (host-side count)"""
    n = len(rows)
    db, dc = F.DeviceTensor.from_numpy(rows), F.DeviceTensor.from_numpy(cls)
    wsb = F._lib.load().frcnn_nms_workspace_bytes(n)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    pick = F.DeviceTensor.from_numpy(np.full(n + 64, SENTINEL, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(2, SENTINEL, np.int32))
    F._lib.call("frcnn_nms_device_classes", F.ptr(db), n, rows.shape[1], C.c_float(thr), 0, 0, F.ptr(dc), F.ptr(pick), F.ptr(cnt),
                F.ptr(ws), wsb, F.stream_ptr())
    k, host = cnt.numpy(), pick.numpy()
    assert 0 <= k[0] <= n and k[1] == SENTINEL and np.all(host[k[0]:] == SENTINEL)
    return host[:k[0]].tolist()


def _batch(F, segments, n_cap, thr, classes=None):
    """frcnn_nms_device_batch over `segments` (arrays of rows; row_stride = n_cap + 37, NaN behind every segment's rows) ->
    the pick list of every segment.  Checks the sentinels behind each segment's picks and behind the arrays, and that the
    boxes are unchanged."""
    B, stride = len(segments), n_cap + 37
    boxes = np.concatenate([_padded(s.reshape(-1, 4), stride) for s in segments])
    counts = np.array([len(s) for s in segments], np.int32)
    dc = None
    if classes is not None:
        cls = np.zeros(B * stride, np.int32)
        for b, c in enumerate(classes):
            cls[b * stride:b * stride + len(c)] = c
        dc = F.DeviceTensor.from_numpy(cls)
    db, ndev = F.DeviceTensor.from_numpy(boxes), F.DeviceTensor.from_numpy(counts)
    wsb = F._lib.load().frcnn_nms_batch_workspace_bytes(B, n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    pick = F.DeviceTensor.from_numpy(np.full(B * stride + 64, SENTINEL, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(B + 1, SENTINEL, np.int32))
    F._lib.call("frcnn_nms_device_batch", F.ptr(db), B, stride, n_cap, F.ptr(ndev), 4, C.c_float(thr), 0, 0, F.ptr(dc), F.ptr(pick),
                F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
    k, host = cnt.numpy(), pick.numpy()
    assert k[B] == SENTINEL and np.all(host[B * stride:] == SENTINEL)
    assert _same_bytes(db.numpy(), boxes), "the boxes changed"
    if dc is not None:
        assert np.array_equal(dc.numpy(), cls)
    out = []
    for b in range(B):
        assert 0 <= k[b] <= counts[b], "segment %d" % b
        assert np.all(host[b * stride + k[b]:(b + 1) * stride] == SENTINEL), "segment %d: stores behind its %d picks" % (b, k[b])
        out.append(host[b * stride:b * stride + k[b]].tolist())
    return out


def _differences(got, want, prob):
    """for the message of a failed comparison: the sorted positions (group, offset) whose fate differs"""
    pos_of = {int(r) + 1: p for p, r in enumerate(prob["row_of"])}
    diff = sorted(pos_of[i] for i in set(got) ^ set(want) if i in pos_of)
    return "%d picks for %d; positions that differ (group, offset): %s" % (len(got), len(want), [(p // 64, p % 64) for p in diff[:24]])


# ---- the single problem ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", NP.CLOSED_FORM, ids=lambda p: p["name"])
def test_table_entry_equals_its_closed_form_and_the_oracle(F, O, prob):
    got = F.nms(prob["rows"], prob["thr"]).tolist()
    assert got == prob["expect"], _differences(got, prob["expect"], prob)
    assert got == O.nms(prob["rows"], prob["thr"]).tolist()


def test_zero_area_boxes_follow_the_oracle(F, O):
    d = NP.DEGENERATE
    want = O.nms(d["rows"], d["thr"]).tolist()
    assert want == d["expect"] == [4, 3]
    assert F.nms(d["rows"], d["thr"]).tolist() == want
    assert _device_n(F, d["rows"], 64, d["thr"]) == want


def test_scan_case_in_every_key_mode(F, O):
    rows, thr = S["rows"], S["thr"]
    b5 = np.concatenate([rows, rows[:, 3:4]], 1)
    got = F.nms(b5, thr, 5).tolist()                                  # a key column that repeats max-y
    assert got == S["expect"], _differences(got, S["expect"], S)
    assert got == O.nms(b5, thr, 2, 5).tolist()
    assert F.nms(b5, thr, b5[:, 4]).tolist() == S["expect"]           # a tensor: max-y
    assert _device_n(F, b5, S["n"], thr, key_mode=2, key_col=5) == S["expect"]
    # 'area': the widths differ (pairs share a slot, the chain is wider), so the order is another one: the oracle only
    want = O.nms(rows, thr, 1).tolist()
    assert want != S["expect"] and len(want) > 4000
    assert F.nms(rows, thr, "area").tolist() == want
    assert _device_n(F, rows, S["n"], thr, key_mode=1) == want


# ---- the row count in device memory, a larger capacity ---------------------------------------------------------------
def test_scan_case_with_device_side_count_and_larger_pitch(F):
    n_cap = S["n"] + 1000
    assert NP.cdiv(n_cap, 64) > NP.cdiv(S["n"], 64)                   # the mask's pitch is not the run's word count
    got = _device_n(F, S["rows"], n_cap, S["thr"])
    assert got == S["expect"], _differences(got, S["expect"], S)


@pytest.mark.parametrize("prob", NP.EDGE_SIZES, ids=lambda p: p["name"])
def test_edge_sizes_with_device_side_count(F, prob):
    got = _device_n(F, prob["rows"], 512, prob["thr"])
    assert got == prob["expect"], _differences(got, prob["expect"], prob)
    assert _device_n(F, prob["rows"], prob["n"], prob["thr"]) == prob["expect"]


# ---- segments --------------------------------------------------------------------------------------------------------
def test_batch_of_six_segments_in_either_order(F):
    probs = [S, NP.ALL_KEPT, NP.ONE_KEPT, NP.CHAIN_ALONE, NP.EQUAL_KEYS, None]
    segs = [p["rows"] if p else np.zeros((0, 4), np.float32) for p in probs]
    want = [p["expect"] if p else [] for p in probs]
    got = _batch(F, segs, S["n"], NP.THR)
    for b, p in enumerate(probs):
        assert got[b] == want[b], "segment %d (%s): %s" % (b, p["name"] if p else "empty", _differences(got[b], want[b], p) if p else got[b])
    back = _batch(F, segs[::-1], S["n"], NP.THR)
    assert back == got[::-1]


# ---- classes ---------------------------------------------------------------------------------------------------------
def test_class_aware_scan_case(F):
    cls, expect = NP.with_classes(S)
    assert len(expect) > len(S["expect"])
    one = np.ones(S["n"], np.int32)
    got = _device_classes(F, S["rows"], S["thr"], cls)
    assert got == expect, _differences(got, expect, S)
    assert _device_classes(F, S["rows"], S["thr"], one) == S["expect"]
    assert _device_n(F, S["rows"], S["n"] + 1000, S["thr"], cls=cls) == expect
    both = _batch(F, [S["rows"], S["rows"]], S["n"], S["thr"], classes=[cls, one])
    assert both[0] == expect, _differences(both[0], expect, S)
    assert both[1] == S["expect"], _differences(both[1], S["expect"], S)


# ---- the same answer every time --------------------------------------------------------------------------------------
def test_scan_case_repeats(F):
    """the scan's waves exchange data through LDS behind bare barriers only: a race would show as runs that differ"""
    runs = [F.nms(S["rows"], S["thr"]).tolist() for _ in range(3)]
    assert runs[0] == S["expect"], _differences(runs[0], S["expect"], S)
    assert runs[1] == runs[0] and runs[2] == runs[0]
