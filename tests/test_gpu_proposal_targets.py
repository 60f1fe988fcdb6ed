"""frcnn_proposal_targets_batch on the device against the numpy restatement of tests/proposal_targets_ref.py, on sentinel-filled
buffers: counts, src, gt_idx, cctarget, roi, iou and the x / y targets are exact (the same fp64 operations); the w / h targets go
through log(), the device's and numpy's each within 1 ulp of the true value, so they differ by at most 2 fp64 ulp, which moves the
rounded float by at most one step: within 1 fp32 ulp.  Nothing is stored behind row F + Bq or in another segment's slice."""
import ctypes as C

import numpy as np
import pytest

import proposal_targets_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
OUT = (("roi", np.float64, 4), ("crtarget", np.float32, 4), ("cctarget", np.float32, 1), ("src", np.int32, 1), ("gt_idx", np.int32, 1),
       ("iou", np.float64, 1))
SCALARS = ("include_gt", "fg_iou", "bg_lo", "bg_hi", "fg_quota", "batch", "bgclass", "seed", "r_cap")


def launch(F, segs, out_stride=None, extra_rows=3, **override):
    """One call on the segments `segs` (cases that share the kernel's scalars), every output buffer filled with SENT bytes and
    `extra_rows` rows longer than the call may use -> (rc, dict of host arrays incl. counts (B + 1) x 4, launches of class rpn)"""
    B = len(segs)
    p = dict((k, segs[0][k]) for k in SCALARS)
    p.update(override)
    assert all(s[k] == segs[0][k] for s in segs for k in SCALARS)
    stride = max([len(s["rect"]) for s in segs] + [len(s["pick"]) for s in segs] + [p["r_cap"], 1])
    gstride = max([len(s["gt_rect"]) for s in segs] + [1])
    rect = np.zeros((B, stride, 4), np.float64); pick = np.zeros((B, stride), np.int64)
    gt = np.zeros((B, gstride, 4), np.float64); gcls = np.zeros((B, gstride), np.int32)
    for b, s in enumerate(segs):
        rect[b, :len(s["rect"])] = s["rect"]; pick[b, :len(s["pick"])] = s["pick"]
        gt[b, :len(s["gt_rect"])] = s["gt_rect"]; gcls[b, :len(s["gt_class"])] = s["gt_class"]
    out_stride = int(p["batch"] if out_stride is None else out_stride)
    rows = B * max(out_stride, 1) + extra_rows
    dev = dict((name, F.DeviceTensor.from_numpy(np.full(rows * n * np.dtype(dt).itemsize, SENT, np.uint8).view(dt)
                                                .reshape((rows, n) if n > 1 else (rows,)))) for name, dt, n in OUT)
    counts = F.DeviceTensor.from_numpy(np.full((B + 1) * 16, SENT, np.uint8).view(np.int32).reshape(B + 1, 4))
    d_rect, d_pick, d_gt, d_gc = (F.DeviceTensor.from_numpy(a) for a in (rect, pick, gt, gcls))
    r_dev = F.DeviceTensor.from_numpy(np.array([s["r_dev"] for s in segs], np.int32))
    G_host = (C.c_int * B)(*[len(s["gt_rect"]) for s in segs])
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        rc = F._lib.load().frcnn_proposal_targets_batch(
            F.ptr(d_rect), F.ptr(d_pick), stride, F.ptr(r_dev), int(p["r_cap"]), F.ptr(d_gt), F.ptr(d_gc), gstride, G_host,
            override.get("B", B), 1 if p["include_gt"] else 0, float(p["fg_iou"]), float(p["bg_lo"]), float(p["bg_hi"]), int(p["fg_quota"]),
            int(p["batch"]), int(p["bgclass"]), C.c_uint(int(p["seed"]) & 0xFFFFFFFF), F.ptr(dev["roi"]), F.ptr(dev["crtarget"]),
            F.ptr(dev["cctarget"]), F.ptr(dev["src"]), F.ptr(dev["gt_idx"]), F.ptr(dev["iou"]), out_stride, F.ptr(counts),
            F.stream_ptr())
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    host = dict((k, t.numpy()) for k, t in dev.items())
    host["counts"] = counts.numpy()
    return rc, host, list(la)[F._lib.KC_NAMES.index("rpn")], sum(la)


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == SENT))


def ulp_steps(a, b):
    """the distance of two float32 arrays in representable steps (equal signs and finite values, or equal bits)"""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def check_segment(host, b, out_stride, case, seg_index=None):
    want = R.targets_ref(case, b if seg_index is None else seg_index)
    got_counts = tuple(int(v) for v in host["counts"][b])
    assert got_counts == want["counts"], (case["name"], got_counts, want["counts"])
    S = want["counts"][2] + want["counts"][3]
    lo = b * out_stride
    for name in ("src", "gt_idx", "cctarget", "roi", "iou"):
        g, w = host[name][lo:lo + S], want[name]
        assert g.reshape(w.shape).view(np.uint8).tobytes() == np.ascontiguousarray(w).view(np.uint8).tobytes(), (case["name"], name)
    g, w = host["crtarget"][lo:lo + S], want["crtarget"]
    assert g[:, :2].tobytes() == w[:, :2].tobytes(), (case["name"], "x / y targets")
    same_nan = np.isnan(g[:, 2:]) & np.isnan(w[:, 2:])
    steps = np.where(same_nan, 0, ulp_steps(g[:, 2:], w[:, 2:]))
    assert steps.max(initial=0) <= 1, (case["name"], "w / h targets", int(steps.max()))
    for name, _, _ in OUT:   # nothing behind row S of the segment's slice
        assert untouched(host[name][lo + S:lo + out_stride]), (case["name"], name, "rows behind F + Bq")
    return S


CASES = R.rule_cases() + R.size_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_restatement(F, case):
    rc, host, launches, _ = launch(F, [case])
    assert rc == 0, F._lib.load().frcnn_last_error()
    check_segment(host, 0, case["batch"], case)
    for name, _, _ in OUT:   # ... nor behind the call's rows
        assert untouched(host[name][case["batch"]:]), name
    assert untouched(host["counts"][1:])
    assert launches == 1


def test_public_function(F):
    case = dict((c["name"], c) for c in R.rule_cases())["cut_both_0"]
    want = R.targets_ref(case)
    got = F.proposal_targets(case["rect"], case["pick"], case["r_dev"], case["gt_rect"], case["gt_class"], case["bgclass"],
                             include_gt=case["include_gt"], fg_iou=case["fg_iou"], bg_iou=(case["bg_lo"], case["bg_hi"]),
                             fg_quota=case["fg_quota"], batch=case["batch"], seed=case["seed"])
    assert got["counts"] == want["counts"]
    for name in ("src", "gt_idx", "cctarget", "roi", "iou"):
        assert got[name].tobytes() == want[name].tobytes(), name
    assert ulp_steps(got["crtarget"], want["crtarget"]).max() <= 1
    with pytest.raises(F.FrcnnError):
        F.proposal_targets(case["rect"], case["pick"], 5, case["gt_rect"], case["gt_class"], 21, fg_quota=9, batch=8)
    with pytest.raises(ValueError):
        F.proposal_targets(case["rect"], [len(case["rect"]) + 1], 1, case["gt_rect"], case["gt_class"], 21)


def test_segments_are_independent_and_runs_repeat(F):
    """B = 3 with different counts, one segment empty: every segment equals its own B = 1 run bit for bit (a segment's key uses its
    index, so the B = 1 run of segment b is the restatement at b -- and, for b = 0, a launch of its own); a second run gives the
    same bits; a longer out_stride moves the slices and nothing else"""
    segs = [dict(c, r_cap=300) for c in R.batch_cases()]
    rc, host, launches, _ = launch(F, segs)
    assert rc == 0 and launches == 1
    stride = segs[0]["batch"]
    S = [check_segment(host, b, stride, s) for b, s in enumerate(segs)]
    assert S[1] == 0 and tuple(host["counts"][1]) == (0, 0, 0, 0) and S[0] > 0 and S[2] > 0
    assert untouched(host["counts"][3:])
    rc2, again, _, _ = launch(F, segs)
    assert rc2 == 0 and all(host[k].tobytes() == again[k].tobytes() for k in host)
    rc1, alone, _, _ = launch(F, segs[:1])
    assert rc1 == 0
    for name, _, _ in OUT:
        assert alone[name][:S[0]].tobytes() == host[name][:S[0]].tobytes(), name
    rc3, wide, _, _ = launch(F, segs, out_stride=stride + 5)
    assert rc3 == 0
    for b in range(3):
        assert check_segment(wide, b, stride + 5, segs[b]) == S[b]
    # the neighbours do not matter: segment 2 between two other segments
    other = [segs[2], segs[0], segs[2]]
    rc4, mixed, _, _ = launch(F, other)
    assert rc4 == 0
    check_segment(mixed, 2, stride, segs[2])
    check_segment(mixed, 1, stride, segs[0])


def test_every_segment_equals_its_own_single_launch(F):
    """A segment's rows depend on its index only through the keys, and the keys only decide which rows of a class over its quota
    stay: with quotas nothing exceeds, each segment of the B = 3 launch equals the B = 1 launch on its data bit for bit -- every
    output array --; with quotas that cut, the B = 1 launch (index 0) has the same four counts, and which rows stay is the
    restatement's at the segment's index (test_segments_are_independent_and_runs_repeat)."""
    for quota, batch in ((400, 800), (10, 40)):
        segs = [dict(c, r_cap=300, fg_quota=quota, batch=batch) for c in R.batch_cases()]
        rc, host, _, _ = launch(F, segs)
        assert rc == 0
        for b, s in enumerate(segs):
            rc1, alone, _, _ = launch(F, [s])
            assert rc1 == 0 and alone["counts"][0].tolist() == host["counts"][b].tolist()
            S = int(host["counts"][b][2] + host["counts"][b][3])
            if quota == 400:
                assert S == int(host["counts"][b][0] + host["counts"][b][1])      # nothing was cut
                for name, _, _ in OUT:
                    assert alone[name][:S].tobytes() == host[name][b * batch:b * batch + S].tobytes(), (b, name)


REFUSALS = [("B negative", dict(B=-1)), ("B too large", dict(B=65536)), ("r_cap + 64 > 4096", dict(r_cap=4033)),
            ("r_cap negative", dict(r_cap=-1)), ("bg_hi > fg_iou", dict(bg_hi=0.6)), ("bg_lo > bg_hi", dict(bg_lo=0.55, bg_hi=0.5)),
            ("threshold NaN", dict(fg_iou=float("nan"))), ("batch < 1", dict(batch=0, fg_quota=0)), ("fg_quota negative", dict(fg_quota=-1)),
            ("fg_quota > batch", dict(fg_quota=33)), ("out_stride < batch", dict(out_stride=31)), ("bgclass < 1", dict(bgclass=0))]


@pytest.mark.parametrize("what,bad", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_launch(F, what, bad):
    case = dict((c["name"], c) for c in R.rule_cases())["cut_both_0"]
    bad = dict(bad)
    out_stride = bad.pop("out_stride", 32)
    if bad.get("r_cap", 0) > 4000:      # (a pick array long enough for the cap that is refused)
        case = dict(case, pick=np.resize(case["pick"], 4033))
    rc, host, _, total = launch(F, [dict(case, batch=32)], out_stride=out_stride, **bad)
    assert rc != 0 and F._lib.load().frcnn_last_error(), what
    assert total == 0, "a refused call launched something"
    assert all(untouched(v) for v in host.values()), what


def test_ground_truth_counts_and_pointers_are_checked(F):
    case = dict((c["name"], c) for c in R.rule_cases())["cut_both_0"]
    L = F._lib.load()
    d = F.DeviceTensor.from_numpy(np.full(4096, SENT, np.uint8))
    one = (C.c_int * 1)

    def call(G=4, gt_stride=4, rect=True, gt=True, out=True, r_dev=True, ghost=True, align=0):
        p = lambda on: C.c_void_p(d.ptr) if on else None
        return L.frcnn_proposal_targets_batch(p(rect), p(rect), 8, p(r_dev), 8, p(gt), p(gt), gt_stride, one(G) if ghost else None, 1, 1,
                                              0.5, 0.0, 0.5, 2, 4, 21, 0, C.c_void_p(d.ptr + 1024 + align), C.c_void_p(d.ptr + 2048), p(out),
                                              p(out), p(out), p(out), 4, C.c_void_p(d.ptr + 3072), F.stream_ptr())
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        for kw in (dict(G=65, gt_stride=65), dict(G=-1), dict(G=5, gt_stride=4), dict(rect=False), dict(gt=False), dict(out=False),
                   dict(r_dev=False), dict(ghost=False), dict(align=8)):
            assert call(**kw) != 0, kw
            assert L.frcnn_last_error()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    assert sum(la) == 0, "a refused call launched something"
    assert untouched(d.numpy())
    assert L.frcnn_proposal_targets_batch(None, None, 0, None, 0, None, None, 0, None, 0, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None,
                                          None, None, None, 0, None, None) == 0   # B = 0: nothing to do, nothing to check
