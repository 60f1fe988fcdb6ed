"""frcnn_eval_match_batch and frcnn_eval_conf_rows (include/frcnn_hip_eval.h) on sentinel-filled buffers against the numpy
restatement (tests/eval_match_ref.py: the literal greedy loop of evaluation.mean_average_precision).  Every int is exact and the
overlaps are compared bit for bit: the kernel's fp64 arithmetic is Rect.IoU's, one rounding per operation.
  * the hand cases, one rule each; all of them as the frames of ONE chunk as well
  * sizes: n = 1, 63, 64, 65 (a wave), 255 ... 257 (a workgroup of the first launch), 16 384 and 22 576 (no row cap: a frame of the all-class test at 0.05 has that capacity), 16 500 in a
    launch of 64 frames (64 workgroups a frame: the first launch strides); G = 1, 4, 5 (a workgroup of
    the second launch holds four boxes), 64, 65, 1 024 (the cap); T = 1, 10, 16; a row stride above n; B = 1, 8, 65 (a launch carries
    64 frames).  The design has no tiers: no boundary beyond these
  * selection: sel_row from frcnn_topk_select at M < n is the restatement on w[keep_best(conf, M)]; M >= n is the identity
  * nothing is written behind a frame's rows; two runs give identical bytes; refused calls leave the outputs untouched"""
import ctypes as C

import numpy as np
import pytest

import eval_match_ref as R

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
IOU_FILL = np.array([FILL, FILL], np.int32).view(np.float64)[0]


def _rec(F, frames, row_stride):
    from frcnn_amd.nms import winner_table
    B = len(frames)
    rec = np.full((B, row_stride + 1, 16), np.nan, np.float64)      # (the records behind a frame's winners: never read)
    for b, fr in enumerate(frames):
        n = len(fr["classes"])
        rec[b, :n + 1] = winner_table(fr["rects"], fr["classes"], fr["conf"])
        rec[b, 0].view(np.int32)[:4] = fr.get("counts", (n,) * 4)
    return rec


def _run(F, frames, thr, row_stride=None, M=None, with_iou=True, T=None, rec=None):
    """-> (return code, match int32[B][row_stride + 2][4], iou float64[B][row_stride] or None, the selected rows per frame or None)
    on buffers prefilled with FILL"""
    L = F._lib.load()
    B = len(frames)
    if row_stride is None:
        row_stride = max([len(fr["classes"]) for fr in frames] + [0])
    rec = _rec(F, frames, row_stride) if rec is None else rec
    d_rec = F.DeviceTensor.from_numpy(rec)
    row0 = np.concatenate([[0], np.cumsum([len(fr["gt_classes"]) for fr in frames])]).astype(np.int64)
    G = int(row0[-1])
    gr = np.concatenate([np.asarray(fr["gt_rects"], np.float64).reshape(-1, 4) for fr in frames] + [np.zeros((1, 4))])
    gc = np.concatenate([np.asarray(fr["gt_classes"], np.int32).reshape(-1) for fr in frames] + [np.zeros(1, np.int32)])
    d_gr, d_gc = F.DeviceTensor.from_numpy(gr), F.DeviceTensor.from_numpy(gc)
    match = F.DeviceTensor.from_numpy(np.full((B, row_stride + 2, 4), FILL, np.int32))
    iou = F.DeviceTensor.from_numpy(np.full((B, max(row_stride, 1)), IOU_FILL, np.float64)) if with_iou else None
    s = F.stream_ptr()
    sel = kd = None
    kcap = 0
    if M is not None:
        kcap = min(row_stride, M)
        conf = F.DeviceTensor.from_numpy(np.full((B, row_stride), np.float32(7.0)))
        cnt = F.DeviceTensor.from_numpy(np.full(B + 1, FILL, np.int32))
        sel = F.DeviceTensor.from_numpy(np.full((B, kcap), FILL, np.int32))
        kd = F.DeviceTensor.from_numpy(np.full(B, FILL, np.int32))
        wsb = L.frcnn_topk_select_workspace_bytes(B, row_stride)
        ws = F.DeviceTensor.empty((wsb,), np.uint8)
        F._lib.call("frcnn_eval_conf_rows", F.ptr(d_rec), B, row_stride, F.ptr(conf), F.ptr(cnt), s)
        hc, hn = conf.numpy(), cnt.numpy()
        for b, fr in enumerate(frames):      # the confidence column and the count, and nothing behind them
            n = len(fr["classes"])
            assert hn[b] == n and hc[b, :n].tobytes() == np.asarray(fr["conf"], np.float32).tobytes() and (hc[b, n:] == 7.0).all()
        assert hn[B] == FILL
        F._lib.call("frcnn_topk_select", F.ptr(conf), B, row_stride, row_stride, F.ptr(cnt), M, F.ptr(sel), kcap, F.ptr(kd), F.ptr(ws),
                    wsb, s)
    t = (C.c_double * max(len(thr), 1))(*thr)
    code = L.frcnn_eval_match_batch(F.ptr(d_rec), B, row_stride, F.ptr(sel), kcap, F.ptr(kd), F.ptr(d_gr), F.ptr(d_gc),
                                    (C.c_longlong * (B + 1))(*[int(v) for v in row0]), t, len(thr) if T is None else T,
                                    F.ptr(match), F.ptr(iou), s)
    rows = None
    if M is not None:
        hs, hk = sel.numpy(), kd.numpy()
        rows = [hs[b, :hk[b]].astype(np.int64) for b in range(B)]
    return code, match.numpy(), iou.numpy() if with_iou else None, rows


def _check(frames, thr, got, iou, sel=None, tag=""):
    """every frame's table against the restatement; FILL everywhere behind its rows"""
    tps = fps = 0
    for b, fr in enumerate(frames):
        want, wiou = R.table(fr, thr, None if sel is None else sel[b])
        k = len(want) - 2
        assert got[b, :k + 2].tolist() == want.tolist(), "%s frame %d" % (tag, b)
        assert (got[b, k + 2:] == FILL).all(), "%s frame %d: written behind row %d" % (tag, b, k)
        if iou is not None:
            assert iou[b, :k].tobytes() == wiou.tobytes(), "%s frame %d: the overlaps" % (tag, b)
            assert iou[b, k:].tobytes() == np.full(iou.shape[1] - k, IOU_FILL).tobytes(), "%s frame %d: iou behind row %d" % (tag, b, k)
        tps += int((want[2:, 2] & 1).sum()); fps += int(k - (want[2:, 2] & 1).sum())
    return tps, fps


@pytest.mark.parametrize("case", R.HAND, ids=[c["name"] for c in R.HAND])
def test_hand_cases(F, case):
    code, got, iou, _ = _run(F, [case], case["thr"], row_stride=len(case["classes"]) + 3)
    assert code == 0
    n = len(case["classes"])
    assert got[0, 1].tolist() == [n, len(case["gt_classes"]), len(case["thr"]), n]
    assert got[0, 2:2 + n, 2].tolist() == case["tp"] and got[0, 2:2 + n, 3].tolist() == case["gt"]
    assert iou[0, :n].tolist() == case["iou"]
    _check([case], case["thr"], got, iou)


def test_hand_cases_as_one_chunk(F):
    """the fourteen cases as the frames of one chunk at the ten thresholds of the 0.5 ... 0.95 range: a frame's result does not
    depend on its neighbours, and the frames without winners or without ground truth sit between the others"""
    code, got, iou, _ = _run(F, R.HAND, R.IOU_RANGE, row_stride=5)
    assert code == 0
    _check(R.HAND, R.IOU_RANGE, got, iou)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_rows_around_a_wave_and_a_workgroup(F, n):
    fr = R.frame(n, n, 7)
    code, got, iou, _ = _run(F, [fr], [0.5, 0.7], row_stride=n + (n % 3))
    assert code == 0
    _check([fr], [0.5, 0.7], got, iou)


@pytest.mark.parametrize("G", [1, 4, 5, 64, 65, 1024])
def test_boxes_up_to_the_cap(F, G):
    fr = R.frame(100 + G, 90, G, ncls=3)
    code, got, iou, _ = _run(F, [fr], [0.5])
    assert code == 0
    tps, fps = _check([fr], [0.5], got, iou)
    assert tps > 0 and fps > 0


@pytest.mark.parametrize("T", [1, 10, 16])
def test_thresholds(F, T):
    thr = [round(0.2 + 0.05 * i, 2) for i in range(T)]
    frames = [R.frame(200 + T + b, 120, 9) for b in range(2)]
    code, got, iou, _ = _run(F, frames, thr)
    assert code == 0
    _check(frames, thr, got, iou)
    masks = np.concatenate([got[b, 2:122, 2] for b in range(2)])
    # (one threshold has two masks; several separate the detections into more)
    assert masks.max() < (1 << T) and len(set(masks.tolist())) > (1 if T == 1 else 2), "the thresholds separate the detections"


@pytest.mark.parametrize("n", [16384, 22576])
def test_rows_beyond_a_soft_pass(F, n):
    """16 384 rows, what a soft per-class NMS takes, and 22 576, the capacity of a frame under "all" at 0.05 (1 411 candidates x 16
    rows): there is no row cap; a wave of the second launch walks the frame 353 times"""
    fr = R.frame(9, n, 6)
    code, got, iou, _ = _run(F, [fr], [0.5], row_stride=n + 5)
    assert code == 0
    tps, fps = _check([fr], [0.5], got, iou)
    assert 0 < tps <= 6 and fps > 16000


def test_the_first_launch_strides_over_the_rows(F):
    """a launch of 64 frames has 64 workgroups a frame: 16 384 rows a pass.  One frame with 16 500 winners among 63 small ones,
    under a selection of 16 450 as well (the selected rows stride too)"""
    frames = [R.frame(40 + b, 2 + b % 5, 3) for b in range(64)]
    frames[37] = R.frame(77, 16500, 7)
    code, got, iou, _ = _run(F, frames, [0.5, 0.9], row_stride=16500)
    assert code == 0
    tps, fps = _check(frames, [0.5, 0.9], got, iou)
    assert tps > 0 and fps > 16000
    code, got, iou, rows = _run(F, frames, [0.5], row_stride=16500, M=16450)
    assert code == 0 and len(rows[37]) == 16450
    _check(frames, [0.5], got, iou, sel=[R.keep_best(fr["conf"], 16450) for fr in frames])


@pytest.mark.parametrize("B", [1, 8, 65])
def test_frames(F, B):
    """B = 65: one frame more than a launch carries -- the last frame is a launch group of its own, and is not a small one"""
    frames = [R.frame(300 + b, 3 + (b * 7) % 30, (b * 5) % 9) for b in range(B)]
    frames[-1] = R.frame(399, 150, 12)
    frames[0]["counts"] = (901, 77, 40, len(frames[0]["classes"]))      # (the gather's header travels to row 0)
    code, got, iou, _ = _run(F, frames, [0.5, 0.75], row_stride=160)
    assert code == 0
    tps, fps = _check(frames, [0.5, 0.75], got, iou)
    assert tps > 0 and fps > 0
    assert got[0, 0].tolist() == [901, 77, 40, len(frames[0]["classes"])]


def test_a_winner_count_above_the_stride_is_clamped(F):
    fr = R.frame(5, 40, 6)
    rec = _rec(F, [fr], 40)[:, :11].copy()        # a table of 10 rows whose header still says 40
    code, got, iou, _ = _run(F, [fr], [0.5], row_stride=10, rec=rec)
    assert code == 0
    short = dict(fr, rects=fr["rects"][:10], classes=fr["classes"][:10], conf=fr["conf"][:10], counts=(40, 40, 40, 40))
    want, wiou = R.table(short, [0.5])
    want[1, 3] = 10
    assert got[0].tolist() == want.tolist() and iou[0].tobytes() == wiou.tobytes()


@pytest.mark.parametrize("M", [1, 40, 129, 130, 1000])
def test_selection_is_keep_best(F, M):
    frames = [R.frame(500 + b, n, 8) for b, n in enumerate((130, 64, 0, 17))]
    code, got, iou, rows = _run(F, frames, [0.5, 0.8], row_stride=130, M=M)
    assert code == 0
    want_rows = [R.keep_best(fr["conf"], M) for fr in frames]
    assert [r.tolist() for r in rows] == [r.tolist() for r in want_rows]
    _check(frames, [0.5, 0.8], got, iou, sel=want_rows)
    if M >= 130:       # the identity: the tables of a call without a selection
        _, plain, piou, _ = _run(F, frames, [0.5, 0.8], row_stride=130)
        assert plain.tobytes() == got.tobytes() and piou.tobytes() == iou.tobytes()
    else:              # who may claim a box changes with the selection
        assert got[0, 1].tolist() == [min(M, 130), 8, 2, 130]


def test_rows_outside_the_table_are_not_read(F):
    """a caller's sel_row: a row outside the frame's winners is emitted as zeros (overlap -1), nothing is read for it"""
    fr = R.frame(7, 20, 5)
    L = F._lib.load()
    rec = F.DeviceTensor.from_numpy(_rec(F, [fr], 20))
    sel = F.DeviceTensor.from_numpy(np.array([3, -1, 20, 1 << 30, 19], np.int32))
    kd = F.DeviceTensor.from_numpy(np.array([5], np.int32))
    match = F.DeviceTensor.from_numpy(np.full((22, 4), FILL, np.int32))
    iou = F.DeviceTensor.from_numpy(np.full(20, IOU_FILL))
    gr, gc = F.DeviceTensor.from_numpy(fr["gt_rects"]), F.DeviceTensor.from_numpy(fr["gt_classes"])
    assert L.frcnn_eval_match_batch(F.ptr(rec), 1, 20, F.ptr(sel), 5, F.ptr(kd), F.ptr(gr), F.ptr(gc), (C.c_longlong * 2)(0, 5),
                                    (C.c_double * 1)(0.5), 1, F.ptr(match), F.ptr(iou), F.stream_ptr()) == 0
    got, gi = match.numpy(), iou.numpy()
    want, wiou = R.table(fr, [0.5], sel=[3, 19])
    assert got[1].tolist() == [5, 5, 1, 20]
    assert got[[2, 6]].tolist() == want[2:].tolist() and gi[[0, 4]].tobytes() == wiou.tobytes()
    assert not got[3:6].any() and gi[1:4].tolist() == [-1.0] * 3 and (got[7:] == FILL).all()


def test_two_runs_give_identical_bytes_and_the_overlaps_are_optional(F):
    frames = [R.frame(600 + b, 200, 20) for b in range(3)]
    a = _run(F, frames, R.IOU_RANGE)
    b = _run(F, frames, R.IOU_RANGE)
    c = _run(F, frames, R.IOU_RANGE, with_iou=False)
    assert a[0] == b[0] == c[0] == 0
    assert a[1].tobytes() == b[1].tobytes() == c[1].tobytes() and a[2].tobytes() == b[2].tobytes() and c[2] is None


def test_refused_calls_leave_the_outputs_untouched(F):
    frames = [R.frame(700, 30, 5)]
    for kw in (dict(T=17), dict(T=0), dict(thr=[0.5, float("nan")])):
        code, got, iou, _ = _run(F, frames, kw.get("thr", [0.5]), T=kw.get("T"))
        assert code != 0 and (got == FILL).all() and iou.tobytes() == np.full(iou.shape, IOU_FILL).tobytes(), kw
    many = dict(frames[0], gt_rects=np.zeros((1025, 4)), gt_classes=np.ones(1025, np.int32))
    code, got, iou, _ = _run(F, [many], [0.5])
    assert code != 0 and (got == FILL).all()


@pytest.mark.parametrize("M", [None, 25])
def test_eval_match_on_host_arrays(F, M):
    fr = R.frame(800, 60, 9)
    out = F.eval_match(fr["rects"], fr["classes"], fr["conf"], fr["gt_rects"], fr["gt_classes"], R.IOU_RANGE, max_detections=M)
    rows = np.arange(60) if M is None else R.keep_best(fr["conf"], M)
    want, wiou = R.table(fr, R.IOU_RANGE, sel=rows)
    assert out["rows"].tolist() == rows.tolist() and out["n"] == len(rows) and out["winners"] == 60
    assert out["cls"].tolist() == want[2:, 0].tolist() and out["confidence"].tobytes() == fr["conf"][rows].tobytes()
    assert out["tp"].tolist() == want[2:, 2].tolist() and out["gt"].tolist() == want[2:, 3].tolist()
    assert out["iou"].tobytes() == wiou.tobytes()
    with pytest.raises(F.FrcnnError, match="thresholds"):
        F.eval_match(fr["rects"], fr["classes"], fr["conf"], fr["gt_rects"], fr["gt_classes"], [0.5] * 17)
