"""frcnn_roi_hard_keys_batch and frcnn_roi_hard_gather_batch on the device against the numpy restatement of tests/roi_hard_ref.py,
on sentinel-filled buffers.  Both kernels are exact: the keys are fp32 operations rounded one by one (no transcendental, FMA
contraction off), the gather copies bits -- so every comparison is of bytes.  Nothing is stored behind a segment's rows, and a
refused call launches and writes nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import roi_hard_ref as H
from anchor_ops_ref import cnet_losses_ref

pytestmark = pytest.mark.gpu

SENT = 0xA5
U = 2.0 ** -24


def _sent(F, shape, dtype):
    return F.DeviceTensor.from_numpy(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, SENT, np.uint8).view(dtype).reshape(shape))


def _is_sent(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == SENT))


def _profiled(F, fn):
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        rc = fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return rc, list(la)


def _pack(segs, stride, names):
    """the segments' arrays side by side, `stride` rows each; unused rows hold values that would be noticed (NaN / -7)"""
    B = len(segs)
    out = {}
    for name in names:
        a0 = np.asarray(segs[0][name])
        a = np.full((B, stride) + a0.shape[1:], np.nan if a0.dtype.kind == "f" else -7, a0.dtype)
        for b, s in enumerate(segs):
            a[b, :len(s[name])] = s[name]
        out[name] = a
    return out


def keys_launch(F, segs, ncls, n_cap, stride, n_host=None, extra=3, **bad):
    B = len(segs)
    host = _pack(segs, stride, ("roi", "crout", "crtarget", "ccout", "cctarget"))
    dev = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in host.items())
    n_host = [len(s["cctarget"]) for s in segs] if n_host is None else n_host
    cnt = F.DeviceTensor.from_numpy(np.array(list(n_host) + [s["nfg"] for s in segs], np.int32))
    box5 = _sent(F, (B * stride + extra, 5), np.float32); loss = _sent(F, (B * stride + extra,), np.float32)
    a = dict(roi=F.ptr(dev["roi"]), crout=F.ptr(dev["crout"]), crtarget=F.ptr(dev["crtarget"]), ccout=F.ptr(dev["ccout"]),
             cctarget=F.ptr(dev["cctarget"]), B=B, stride=stride, n_cap=n_cap, n_dev=F.ptr(cnt), nfg_dev=C.c_void_p(cnt.ptr + 4 * B),
             ncls=ncls, box5=F.ptr(box5), loss=F.ptr(loss))
    a.update((k[4:], v) for k, v in bad.items())     # arg_NAME = value: what the call is given in place of the good argument
    rc, la = _profiled(F, lambda: F._lib.load().frcnn_roi_hard_keys_batch(
        a["roi"], a["crout"], a["crtarget"], a["ccout"], a["cctarget"], a["B"], a["stride"], a["n_cap"], a["n_dev"], a["nfg_dev"], a["ncls"],
        a["box5"], a["loss"], F.stream_ptr()))
    return rc, box5.numpy(), loss.numpy(), la


def check_keys(F, segs, ncls, n_cap=None, stride=None):
    n_cap = max([len(s["cctarget"]) for s in segs] + [0]) if n_cap is None else n_cap
    stride = max(n_cap, 1) if stride is None else stride
    rc, box5, loss, la = keys_launch(F, segs, ncls, n_cap, stride)
    assert rc == 0
    assert sum(la) == la[F._lib.KC_NAMES.index("rpn")] == (1 if n_cap else 0)
    for b, s in enumerate(segs):
        n = min(len(s["cctarget"]), n_cap)
        wb, wl = H.keys_ref(s["roi"][:n], s["crout"][:n], s["crtarget"][:n], s["ccout"][:n], s["cctarget"][:n], min(s["nfg"], n))
        assert loss[b * stride:b * stride + n].tobytes() == wl.tobytes(), "loss of segment %d" % b
        assert box5[b * stride:b * stride + n].tobytes() == wb.tobytes(), "box5 of segment %d" % b
        assert _is_sent(loss[b * stride + n:(b + 1) * stride]) and _is_sent(box5[b * stride + n:(b + 1) * stride]), "behind row n of segment %d" % b
    assert _is_sent(loss[len(segs) * stride:]) and _is_sent(box5[len(segs) * stride:])
    return loss


@pytest.mark.parametrize("n,ncls", [(0, 2), (1, 17), (63, 201), (64, 2), (65, 17), (1023, 201), (1025, 2), (4096, 17)])
def test_keys_equal_the_restatement_at_every_size(F, n, ncls):
    """three segments a launch -- no, one and only foreground rows -- with the arithmetic edges planted: |z| exactly 1 and next to it,
    a NaN and an inf in crout and in ccout, targets of 0, ncls + 1 and NaN"""
    rng = np.random.RandomState(n + ncls)
    segs = [H.edge_rows(H.random_table(rng, n, nfg, ncls)) for nfg in (0, min(1, n), n)]
    loss = check_keys(F, segs, ncls)
    if n >= 63:
        flat = loss[:3 * n]
        assert np.any(flat == np.inf) and np.any(flat == -np.inf) and not np.any(np.isnan(flat))


@pytest.mark.parametrize("ncls", [2, 17, 201])
def test_keys_segments_of_different_counts_and_a_wider_stride(F, ncls):
    rng = np.random.RandomState(ncls)
    segs = [H.edge_rows(H.random_table(rng, n, nfg, ncls)) for n, nfg in ((300, 70), (0, 0), (257, 257))]
    check_keys(F, segs, ncls, n_cap=300, stride=331)
    # the count is read on the device and clamped: n_dev above n_cap reads n_cap rows, a negative one none
    segs = [H.random_table(rng, 100, 30, ncls) for _ in range(3)]
    rc, box5, loss, _ = keys_launch(F, segs, ncls, 64, 100, n_host=[1000, -5, 64])
    assert rc == 0
    for b, n in enumerate((64, 0, 64)):
        s = segs[b]
        wb, wl = H.keys_ref(s["roi"][:n], s["crout"][:n], s["crtarget"][:n], s["ccout"][:n], s["cctarget"][:n], min(s["nfg"], n))
        assert loss[b * 100:b * 100 + n].tobytes() == wl.tobytes() and box5[b * 100:b * 100 + n].tobytes() == wb.tobytes()
        assert _is_sent(loss[b * 100 + n:(b + 1) * 100]) and _is_sent(box5[b * 100 + n:(b + 1) * 100])


def test_keys_sum_to_the_losses_of_the_objective(F):
    """the sum of the rows' losses is frcnn_cnet_losses' pair: 10 * reg_sum + R * cls_mean.  Bound: a row's fp32 loss is at most 8
    roundings (two a term, three sums, the factor, the final sum) of magnitudes bounded by mag_r = |cls| + 10 * sum|term| away from
    its exact value, so the rows contribute 8 * 2^-24 * sum(mag_r); math.fsum adds no error of its own beyond one rounding."""
    rng = np.random.RandomState(4)
    R, nfg, ncls = 777, 200, 21
    c = H.random_table(rng, R, nfg, ncls)
    rc, _, loss, _ = keys_launch(F, [c], ncls, R, R)
    assert rc == 0
    ref = cnet_losses_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], R, nfg, ncls)
    want = 10.0 * ref["reg_sum"] + R * ref["cls_mean"]
    got = math.fsum(float(v) for v in loss[:R])
    z = (c["crout"][:nfg] - c["crtarget"][:nfg]).astype(np.float64)
    mag = float(np.sum(np.abs(c["ccout"][np.arange(R), c["cctarget"].astype(int) - 1]))
                + 10.0 * np.sum(np.where(np.abs(z) < 1, 0.5 * z * z, np.abs(z) - 0.5)))
    print("sum of the keys %.9g, the objective's %.9g, bound %.3g" % (got, want, 8 * U * mag + 2.0 ** -52 * mag))
    assert abs(got - want) <= 8 * U * mag + 2.0 ** -52 * mag


# ---------------------------------------------------------------------------------------------------------------- gather
OUT = H.TABLE + (("loss", np.float32, 1),)


def gather_launch(F, segs, batch, n_cap, stride, out_stride, extra=3, **bad):
    """segs: dicts with the "all" table, loss, nfg, pick (any length <= stride), count, n"""
    B = len(segs)
    names = [name for name, _, _ in H.TABLE] + ["loss"]
    host = _pack(segs, stride, names)
    dev = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in host.items())
    pick = np.full((B, stride), -9, np.int64)
    for b, s in enumerate(segs):
        pick[b, :len(s["pick"])] = s["pick"]
    d_pick = F.DeviceTensor.from_numpy(pick)
    cnt = F.DeviceTensor.from_numpy(np.array([s["count"] for s in segs] + [s["n"] for s in segs] + [s["nfg"] for s in segs], np.int32))
    rows = B * max(out_stride, 1) + extra
    out = dict((name, _sent(F, (rows, k) if k > 1 else (rows,), dt)) for name, dt, k in OUT)
    counts = _sent(F, (B + 1, 4), np.int32)
    a = dict(pick=F.ptr(d_pick), count=F.ptr(cnt), batch=batch, B=B, stride=stride, n_cap=n_cap, n_dev=C.c_void_p(cnt.ptr + 4 * B),
             nfg_dev=C.c_void_p(cnt.ptr + 8 * B), out_stride=out_stride, counts=F.ptr(counts), roi_out=F.ptr(out["roi"]),
             crtarget_out=F.ptr(out["crtarget"]), roi=F.ptr(dev["roi"]))
    a.update((k[4:], v) for k, v in bad.items())     # arg_NAME = value: what the call is given in place of the good argument
    rc, la = _profiled(F, lambda: F._lib.load().frcnn_roi_hard_gather_batch(
        a["pick"], a["count"], a["batch"], a["roi"], F.ptr(dev["crtarget"]), F.ptr(dev["cctarget"]), F.ptr(dev["src"]),
        F.ptr(dev["gt_idx"]), F.ptr(dev["iou"]), F.ptr(dev["loss"]), a["B"], a["stride"], a["n_cap"], a["n_dev"], a["nfg_dev"],
        a["roi_out"], a["crtarget_out"], F.ptr(out["cctarget"]), F.ptr(out["src"]), F.ptr(out["gt_idx"]), F.ptr(out["iou"]),
        F.ptr(out["loss"]), a["out_stride"], a["counts"], F.stream_ptr()))
    host_out = dict((k, t.numpy()) for k, t in out.items())
    host_out["counts"] = counts.numpy()
    return rc, host_out, la


def check_gather(F, segs, batch, n_cap, stride=None, out_stride=None):
    stride = max(n_cap, 1) if stride is None else stride
    out_stride = min(batch, n_cap) + 2 if out_stride is None else out_stride
    rc, got, la = gather_launch(F, segs, batch, n_cap, stride, out_stride)
    assert rc == 0
    assert sum(la) == la[F._lib.KC_NAMES.index("rpn")] == 1
    for b, s in enumerate(segs):
        n = min(max(s["n"], 0), n_cap)
        want = H.gather_ref(s["pick"], min(max(s["count"], 0), n_cap), batch, n, min(s["nfg"], n), s, s["loss"])
        assert tuple(got["counts"][b]) == want["counts"], (b, tuple(got["counts"][b]), want["counts"])
        S = want["counts"][0] + want["counts"][1]
        lo = b * out_stride
        for name, _, _ in OUT:
            assert got[name][lo:lo + S].tobytes() == want[name].tobytes(), "%s of segment %d" % (name, b)
            assert _is_sent(got[name][lo + S:lo + out_stride]), "%s behind row F + Bq of segment %d" % (name, b)
    for name, _, _ in OUT:
        assert _is_sent(got[name][len(segs) * out_stride:])
    assert _is_sent(got["counts"][len(segs):])
    return got


def _gather_seg(rng, n, nfg, count, ncls=5, order=None, nominal=None):
    c = H.random_table(rng, n, nfg, ncls)
    seg = H.table_of(c)
    seg.update(loss=rng.randn(n).astype(np.float32), nfg=nfg, n=n if nominal is None else nominal, count=count,
               pick=(rng.permutation(n) + 1 if order is None else np.asarray(order)).astype(np.int64))
    return seg


@pytest.mark.parametrize("batch,n", [(1, 300), (128, 300), (4096, 4096), (128, 1025)])
def test_gather_equals_the_restatement_at_every_count(F, batch, n):
    """one launch: a segment for each count in {0, 1, batch - 1, batch, batch + 1, n} (those that fit n), on random distinct picks"""
    rng = np.random.RandomState(batch + n)
    counts = sorted(set(c for c in (0, 1, batch - 1, batch, batch + 1, n) if 0 <= c <= n))
    segs = [_gather_seg(rng, n, n // 3, c) for c in counts]
    got = check_gather(F, segs, batch, n)
    assert [int(got["counts"][b][0] + got["counts"][b][1]) for b in range(len(segs))] == [min(c, batch) for c in counts]


def test_gather_foreground_only_background_only_and_picks_outside(F):
    rng = np.random.RandomState(8)
    n = 200
    fg = rng.permutation(60) + 1; bg = rng.permutation(140) + 61
    segs = [_gather_seg(rng, n, 60, 40, order=np.concatenate([fg, bg])),                 # picks: foreground rows only
            _gather_seg(rng, n, 60, 100, order=np.concatenate([bg, fg])),                # background rows only
            _gather_seg(rng, n, n, 90), _gather_seg(rng, n, 0, 90),                      # a table without background / foreground
            # a pick of 0, of n + 1, a negative and a huge one in the list: skipped, and they do not count towards batch
            _gather_seg(rng, n, 60, 70, order=np.concatenate([[0, n + 1, 5, -3, 1 << 40, 12], rng.permutation(150) + 20])),
            _gather_seg(rng, n, 60, 6, order=[0, n + 1, 0, -1, n + 1, 0]),               # none of the picks is a row
            _gather_seg(rng, 0, 0, 0, nominal=0), _gather_seg(rng, 50, 10, 0),           # a segment without rows / without picks
            _gather_seg(rng, 150, 10, 150, nominal=1000)]                                # (n_dev above n_cap is clamped)
    got = check_gather(F, segs, 64, n, stride=n + 9)
    c = got["counts"]
    assert tuple(c[0]) == (40, 0, 40, n) and tuple(c[1]) == (0, 64, 100, n) and tuple(c[2])[:2] == (64, 0) and tuple(c[3])[:2] == (0, 64)
    assert c[4][0] + c[4][1] == 64 and tuple(c[5]) == (0, 0, 6, n) and tuple(c[6]) == (0, 0, 0, 0) and tuple(c[7]) == (0, 0, 0, 50)


def test_roi_hard_select_equals_the_restatement_end_to_end(F):
    """keys, the library's NMS keyed by the loss, gather -- on boxes with exact duplicates (IoU 1) and rows of equal loss (the tie
    rule: the higher row is picked first)"""
    rng = np.random.RandomState(21)
    for n, nfg, batch, overlap in ((150, 40, 32, 0.5), (150, 0, 150, 0.7), (90, 90, 16, 0.3), (64, 10, 4096, 1.0), (1, 1, 1, 0.7), (0, 0, 8, 0.7)):
        c = H.random_table(rng, n, nfg, 7, span=100.0, dup=0.25, equal_loss=0.25)
        got = F.roi_hard_select(c["roi"], c["crout"], c["crtarget"], c["ccout"], c["cctarget"], nfg, batch=batch, overlap=overlap,
                                src=c["src"], gt_idx=c["gt_idx"], iou=c["iou"])
        box5, loss = H.keys_ref(c["roi"], c["crout"], c["crtarget"], c["ccout"], c["cctarget"], nfg)
        want = H.select_ref(box5, loss, nfg, batch, overlap, H.table_of(c))
        assert got["box5"].tobytes() == box5.tobytes() and got["loss_all"].tobytes() == loss.tobytes()
        assert got["pick"].tolist() == want["pick"].tolist()
        assert got["counts"] == want["counts"]
        for name, _, _ in OUT:
            assert got[name].tobytes() == want[name].tobytes(), name
        if n == 150 and nfg == 40:
            assert len(np.unique(loss)) < n and len(np.unique(c["roi"], axis=0)) < n and want["counts"][2] < n   # ties, duplicates, suppression
        if overlap == 1.0:
            assert want["rows"] == list(range(n))


def test_refused_calls_launch_and_write_nothing(F):
    rng = np.random.RandomState(1)
    seg = H.random_table(rng, 40, 10, 5)
    for bad in (dict(arg_B=-1), dict(arg_B=65536), dict(arg_n_cap=4097), dict(arg_n_cap=-1), dict(arg_stride=39), dict(arg_ncls=0), dict(arg_n_dev=None),
                dict(arg_nfg_dev=None), dict(arg_box5=None), dict(arg_loss=None), dict(arg_roi=None), dict(arg_ccout=None)):
        rc, box5, loss, la = keys_launch(F, [seg], 5, 40, 40, **bad)
        assert rc != 0 and sum(la) == 0 and _is_sent(box5) and _is_sent(loss), bad
    buf = F.DeviceTensor.from_numpy(np.zeros((41, 4), np.float32))
    rc, box5, loss, la = keys_launch(F, [seg], 5, 40, 40, arg_crout=C.c_void_p(buf.ptr + 4))
    assert rc != 0 and sum(la) == 0 and _is_sent(box5) and _is_sent(loss)
    g = _gather_seg(rng, 40, 10, 20)
    for bad in (dict(arg_B=-1), dict(arg_B=65536), dict(arg_n_cap=4097), dict(arg_stride=39), dict(arg_batch=0), dict(arg_out_stride=15), dict(arg_count=None),
                dict(arg_n_dev=None), dict(arg_nfg_dev=None), dict(arg_counts=None), dict(arg_pick=None), dict(arg_roi_out=None)):
        rc, got, la = gather_launch(F, [g], 16, 40, 40, 18, **bad)
        assert rc != 0 and sum(la) == 0 and all(_is_sent(v) for v in got.values()), bad
    buf = F.DeviceTensor.from_numpy(np.zeros((64, 4), np.float64))
    rc, got, la = gather_launch(F, [g], 16, 40, 40, 18, arg_roi_out=C.c_void_p(buf.ptr + 8))
    assert rc != 0 and sum(la) == 0 and all(_is_sent(v) for v in got.values())
    # B = 0 returns at once
    rc, got, la = gather_launch(F, [g], 16, 40, 40, 18, arg_B=0)
    assert rc == 0 and sum(la) == 0 and all(_is_sent(v) for v in got.values())
