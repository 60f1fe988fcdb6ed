"""Soft-NMS on the device (frcnn_soft_nms_batch, cfg.nms).  Kernel level: the exact combinations (hard; linear on plain scores;
gaussian on log-scores) bit for bit against the fp32 restatement of tests/soft_nms_ref.py and, for hard, against
frcnn_nms_device_batch; the two inexact ones (log1pf, expf) against the float64 restatement on margin-filtered inputs, within the
bound derived there.  Counts on both sides of the kernel's breakpoints (512 | 513: one wave in registers | the workgroup with LDS;
2048 | 2049: LDS | global memory).  Detector level (vgg_small, amplified weights, 128x176 frames): the setting off changes nothing
and launches nothing new; under a soft method the winners are the restatement's on the record's own rows."""
import ctypes as C
import math

import numpy as np
import pytest

import soft_nms_ref as R
from test_gpu_detect_batch import _Val, _amplified_weights, _frames, _winner_rows
from test_gpu_proposals import _collect, _launches, _same
from test_soft_nms_host import KINDS, SHAPES, exact_inputs

pytestmark = pytest.mark.gpu
SENT = -7
EXACT = [(R.HARD, 0), (R.HARD, 1), (R.LINEAR, 0), (R.GAUSSIAN, 1)]
SMALL = (0, 1, 2, 63, 64, 65, 257)
BIG = (512, 513, 1000, 2048, 2049)            # one count on each side of each breakpoint, and the issue's 1000
LOG_MIN = math.log(0.001)


def _params(log_domain, overlap=0.3):
    return dict(overlap=overlap, sigma=0.5, min_score=LOG_MIN if log_domain else 0.001)


def _classes(mode, rng, n):
    if mode == "none":
        return None
    if mode == "three":
        return rng.randint(1, 4, n).astype(np.int32)
    return (rng.permutation(n) + 1).astype(np.int32)       # all distinct


def _run(F, rows, B, stride, n_cap, counts, method, P, log_domain, cls=None, score_col=5, score_stride=1, scores=True):
    """frcnn_soft_nms_batch on host arrays (rows: [B * stride][ncols]) -> (pick [B][stride], count [B], score_out [B][stride]
    or None); asserts that the inputs come back unchanged and that the guard tails are untouched."""
    L = F._lib.load()
    ncols = rows.shape[1]
    assert rows.shape[0] == B * stride
    d = F.DeviceTensor.from_numpy(rows)
    ndev = F.DeviceTensor.from_numpy(np.asarray(counts, np.int32))
    dc = F.DeviceTensor.from_numpy(cls) if cls is not None else None
    pick = F.DeviceTensor.from_numpy(np.full(B * stride + 8, SENT, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(B + 1, SENT, np.int32))
    out = F.DeviceTensor.from_numpy(np.full(B * stride * score_stride + 8, SENT, np.float32)) if scores else None
    wsb = L.frcnn_soft_nms_workspace_bytes(B, n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    F._lib.call("frcnn_soft_nms_batch", F.ptr(d), B, stride, n_cap, F.ptr(ndev), ncols, score_col, method, C.c_float(P["overlap"]),
                C.c_float(P["sigma"]), C.c_float(P["min_score"]), log_domain, F.ptr(dc), F.ptr(pick), F.ptr(cnt), F.ptr(out),
                score_stride, F.ptr(ws), wsb, F.stream_ptr())
    pick, cnt = pick.numpy(), cnt.numpy()
    assert np.array_equal(d.numpy().view(np.uint32), rows.view(np.uint32)), "the rows were written"
    assert ndev.numpy().tolist() == list(counts), "the counts were written"
    if cls is not None:
        assert np.array_equal(dc.numpy(), cls), "the classes were written"
    assert cnt[B] == SENT and np.all(pick[B * stride:] == SENT)
    if scores:
        out = out.numpy()
        assert np.all(out[B * stride * score_stride:] == SENT)
        out = out[:B * stride * score_stride].reshape(B, stride, score_stride)
        assert np.all(out[:, :, 1:] == SENT), "stores between the score slots"
        out = out[:, :, 0]
    return pick[:B * stride].reshape(B, stride), cnt[:B], out


def _check_exact(F, rows, B, stride, n_cap, counts, method, log_domain, cls, tag, score_stride=1, overlap=0.3):
    P = _params(log_domain, overlap)
    pick, cnt, out = _run(F, rows, B, stride, n_cap, counts, method, P, log_domain, cls, score_stride=score_stride)
    for b in range(B):
        n = min(counts[b], n_cap)
        seg = slice(b * stride, b * stride + n)
        wp, ws = R.soft_nms_f32(rows[seg], 5, method, P["overlap"], P["sigma"], P["min_score"], log_domain,
                                None if cls is None else cls[seg])
        t = "%s segment %d (n %d)" % (tag, b, n)
        assert int(cnt[b]) == len(wp), "%s: count %d, want %d" % (t, cnt[b], len(wp))
        k = len(wp)
        assert np.array_equal(pick[b, :k], wp), "%s: picks" % t
        assert np.all(pick[b, k:] == SENT), "%s: stores behind the picks" % t
        want = np.full(stride, SENT, np.float32)
        want[wp - 1] = ws
        assert np.array_equal(out[b].view(np.uint32), want.view(np.uint32)), "%s: scores at pick / stores for unpicked rows" % t
    return pick, cnt, out


# ------------------------------------------------------------------------------------------------ kernel level: exact
@pytest.mark.parametrize("kind", KINDS)
def test_exact_combinations_small_counts_against_the_fp32_restatement(F, kind):
    for i, n in enumerate(SMALL):
        for method, log_domain in EXACT:
            for mode in ("none", "three", "distinct"):
                rng = np.random.RandomState(1000 * i + 10 * method + log_domain)
                rows = exact_inputs(kind, 7 * n + 3, n, log_domain)
                n_cap = max(n, 1)
                pad = np.full((n_cap - n + 3, 5), 9.0, np.float32)       # (rows past the count would win if they were read)
                rows = np.concatenate([rows, pad])
                cls = _classes(mode, rng, len(rows))
                _check_exact(F, rows, 1, len(rows), n_cap, [n], method, log_domain, cls,
                             "%s n=%d %s/%d cls=%s" % (kind, n, R.METHODS[method], log_domain, mode))


@pytest.mark.parametrize("n", BIG)
def test_exact_combinations_at_the_breakpoints_against_the_fp32_restatement(F, n):
    for i, (method, log_domain) in enumerate(EXACT):
        mode = ("none", "three", "distinct", "three")[(i + n) % 4]
        kind = ("clustered", "equal_scores", "below_min_score", "one_nan")[(i + n // 2) % 4]
        rng = np.random.RandomState(n + i)
        rows = exact_inputs(kind, n + 31 * i, n, log_domain)
        _check_exact(F, rows, 1, n, n, [n], method, log_domain, _classes(mode, rng, n),
                     "%s n=%d %s/%d cls=%s" % (kind, n, R.METHODS[method], log_domain, mode))


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("mode", ["none", "three", "distinct"])
def test_exact_combinations_in_segments_with_unequal_counts(F, B, mode):
    """an empty segment, a full one, one whose device count exceeds n_cap, counts on both sides of the one-wave bound, a row
    stride above n_cap and a score stride above 1 in the same call; hard also against frcnn_nms_device_batch"""
    n_cap, stride = 600, 611
    counts = [0, n_cap, n_cap + 7, 63, 1, 513, 300, 65][:B] if B > 1 else [n_cap - 1]
    rng = np.random.RandomState(50 + B)
    for i, (method, log_domain) in enumerate(EXACT):
        rows = np.full((B * stride, 5), 9.0, np.float32)
        kinds = [k for k in KINDS if not (method == R.HARD and k == "one_nan")]    # (the bit-matrix NMS has no rule for a NaN key)
        for b in range(B):
            rows[b * stride:b * stride + n_cap] = exact_inputs(kinds[(b + i) % len(kinds)], 100 * B + 10 * b + i, n_cap, log_domain)
        cls = _classes(mode, rng, B * stride)
        tag = "B=%d %s/%d cls=%s" % (B, R.METHODS[method], log_domain, mode)
        pick, cnt, _ = _check_exact(F, rows, B, stride, n_cap, counts, method, log_domain, cls, tag, score_stride=1 + i % 2)
        if method == R.HARD:
            P = dict(_params(log_domain), min_score=-np.inf)
            pick, cnt, _ = _run(F, rows, B, stride, n_cap, counts, method, P, log_domain, cls)
            hp, hc = _hard_nms(F, rows, B, stride, n_cap, counts, P["overlap"], cls)
            assert np.array_equal(cnt, hc) and np.array_equal(pick, hp), "%s: frcnn_nms_device_batch" % tag


def _hard_nms(F, rows, B, stride, n_cap, counts, overlap, cls):
    L = F._lib.load()
    d = F.DeviceTensor.from_numpy(rows)
    ndev = F.DeviceTensor.from_numpy(np.asarray(counts, np.int32))
    dc = F.DeviceTensor.from_numpy(cls) if cls is not None else None
    pick = F.DeviceTensor.from_numpy(np.full(B * stride, SENT, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(B, SENT, np.int32))
    wsb = L.frcnn_nms_batch_workspace_bytes(B, n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    F._lib.call("frcnn_nms_device_batch", F.ptr(d), B, stride, n_cap, F.ptr(ndev), rows.shape[1], C.c_float(overlap), 2, 5, F.ptr(dc),
                F.ptr(pick), F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
    return pick.numpy().reshape(B, stride), cnt.numpy()


@pytest.mark.parametrize("n", [513, 2049, 5000, 16384])
def test_hard_equals_the_bit_matrix_nms_keyed_by_the_score(F, n):
    """with nothing below min_score, method hard is frcnn_nms_device_batch(key_mode 2, key_col 5) bit for bit, with and without
    classes -- up to the largest segment the entry point takes (the global-memory path)"""
    rng = np.random.RandomState(n)
    for log_domain, kind in ((0, "clustered"), (1, "equal_scores")):
        rows = exact_inputs(kind, n + log_domain, n, log_domain)
        for cls in (None, _classes("three", rng, n)):
            P = dict(overlap=0.3, sigma=0.5, min_score=-np.inf)
            pick, cnt, out = _run(F, rows, 1, n, n, [n], R.HARD, P, log_domain, cls)
            hp, hc = _hard_nms(F, rows, 1, n, n, [n], 0.3, cls)
            k = int(cnt[0])
            assert k == int(hc[0]) > 0 and np.array_equal(pick[0, :k], hp[0, :k]), (n, log_domain, cls is None)
            assert np.all(pick[0, k:] == SENT)
            assert np.array_equal(out[0][pick[0, :k] - 1].view(np.uint32), rows[pick[0, :k] - 1, 4].view(np.uint32))


@pytest.mark.parametrize("method,log_domain", [(m, l) for m in (R.HARD, R.LINEAR, R.GAUSSIAN) for l in (0, 1)])
def test_rows_that_do_not_touch_come_back_in_score_order_unchanged(F, method, log_domain):
    """pairwise disjoint boxes, and overlapping boxes of all-distinct classes: any method picks in score order (ties: the higher
    row) and returns every score bit for bit -- expf(-0) and log1pf are never asked for anything but the identity"""
    P = _params(log_domain)
    for n in (65, 513, 2049):
        for kind, mode in (("disjoint", "none"), ("disjoint", "three"), ("clustered", "distinct"), ("equal_scores", "distinct")):
            rows = exact_inputs(kind, n, n, log_domain)
            cls = _classes(mode, np.random.RandomState(n), n)
            pick, cnt, out = _run(F, rows, 1, n, n, [n], method, P, log_domain, cls)
            order = np.lexsort((-np.arange(n), -rows[:, 4]))
            assert int(cnt[0]) == n and np.array_equal(pick[0], order + 1), (n, kind, mode)
            assert np.array_equal(out[0].view(np.uint32), rows[:, 4].view(np.uint32)), (n, kind, mode)


def test_signed_zeros_tie_and_the_higher_row_wins(F):
    """log-probabilities of exactly 0 in both signs: compared as values, -0 equals +0, and the score comes back with its sign"""
    rng = np.random.RandomState(8)
    for n in (5, 64, 700, 2100):
        sc = rng.choice(np.array([0.0, -0.0, -0.25], np.float32), n)
        rows = R.rows5(R.disjoint_boxes(rng, n), sc)
        rows[:, 4] = sc                       # (keeps the sign of the zeros)
        for cls in (None, _classes("three", rng, n)):
            _check_exact(F, rows, 1, n, n, [n], R.GAUSSIAN, 1, cls, "zeros n=%d" % n)


def test_soft_nms_does_not_depend_on_the_segment_slot(F):
    """the same rows in every segment: the same picks and scores in every segment (every path)"""
    for n, method, log_domain in ((300, R.GAUSSIAN, 1), (700, R.LINEAR, 0), (2100, R.GAUSSIAN, 0), (2100, R.LINEAR, 1)):
        B = 8
        rows = exact_inputs("clustered", n, n, log_domain)
        cls = _classes("three", np.random.RandomState(n), n)
        pick, cnt, out = _run(F, np.tile(rows, (B, 1)), B, n, n, [n] * B, method, _params(log_domain), log_domain, np.tile(cls, B))
        assert int(cnt[0]) > 0
        for b in range(1, B):
            assert cnt[b] == cnt[0] and np.array_equal(pick[b], pick[0]), (n, b)
            assert np.array_equal(out[b].view(np.uint32), out[0].view(np.uint32)), (n, b)


def test_soft_nms_argument_errors_launch_nothing(F):
    rows = F.DeviceTensor.zeros((64, 5), np.float32)
    i = F.DeviceTensor.zeros((64,), np.int32)
    p = F.DeviceTensor.zeros((64,), np.int64)
    o = F.DeviceTensor.zeros((64,), np.float32)
    ws = F.DeviceTensor.empty((1 << 20,), np.uint8)
    big = F._lib.load().frcnn_soft_nms_workspace_bytes(1, 4096)
    assert 4096 * 4 <= big <= (1 << 20)
    f = C.c_float
    good = dict(boxes=F.ptr(rows), B=1, stride=16, n_cap=16, n_dev=F.ptr(i), ncols=5, score_col=5, method=2, overlap=f(0.3),
                sigma=f(0.5), min_score=f(0.001), log_domain=0, cls=None, pick=F.ptr(p), count=F.ptr(i), score_out=F.ptr(o),
                score_stride=1, ws=F.ptr(ws), wsb=1 << 20)
    bad = [dict(method=3), dict(method=-1), dict(sigma=f(0.0)), dict(sigma=f(-1.0)), dict(score_col=4), dict(score_col=6),
           dict(ncols=4, score_col=4), dict(B=0), dict(stride=15), dict(n_dev=None), dict(pick=None), dict(count=None),
           dict(n_cap=16385, stride=16385), dict(n_cap=4096, stride=4096, wsb=256), dict(wsb=16)]

    def call(args):
        F._lib.call("frcnn_soft_nms_batch", *(list(args.values()) + [F.stream_ptr()]))

    def errors():
        for t in bad:
            with pytest.raises(F.FrcnnError):
                call(dict(good, **t))
    la = _launches(F, errors)
    assert la["soft_nms"] == 0 and sum(la.values()) == 0, la
    la = _launches(F, lambda: (call(good), call(dict(good, score_out=None))))      # (the counter does count; score_out may be NULL)
    assert la["soft_nms"] == 2


def test_python_surface(F):
    rows = exact_inputs("clustered", 3, 300, 0)
    cls = _classes("three", np.random.RandomState(3), 300)
    for method, log_scores in ((R.LINEAR, False), (R.GAUSSIAN, True), (R.HARD, False)):
        r = rows.copy()
        if log_scores:
            r[:, 4] = np.log(r[:, 4])
        ms = LOG_MIN if log_scores else 0.001
        want = R.soft_nms_f32(r, 5, method, 0.3, 0.5, ms, int(log_scores), cls)
        for boxes, classes in ((r, cls), (F.DeviceTensor.from_numpy(r), F.DeviceTensor.from_numpy(cls))):
            pick, sc = F.soft_nms(boxes, 0.3, 5, method=R.METHODS[method], min_score=ms, log_scores=log_scores, classes=classes)
            assert pick.dtype == np.int64 and sc.dtype == np.float32
            assert np.array_equal(pick, want[0]) and np.array_equal(sc.view(np.uint32), want[1].view(np.uint32))
    pick, sc = F.soft_nms(np.zeros((0, 5), np.float32), 0.3, 5)
    assert pick.shape == (0,) and sc.shape == (0,) and pick.dtype == np.int64 and sc.dtype == np.float32
    with pytest.raises(ValueError):
        F.soft_nms(rows, 0.3, 5, method="soft")


# ------------------------------------------------------------------------------------------------ kernel level: inexact
@pytest.mark.parametrize("method,log_domain", R.INEXACT)
def test_inexact_combinations_against_the_float64_restatement(F, method, log_domain):
    """only inputs whose float64 margin exceeds twice the derived bound (the builder asserts its own discard cap): identical
    picks, scores within the bound"""
    worst = 0.0
    for n in SHAPES:
        for nclasses in (0, 3):
            for c in R.inexact_cases(method, log_domain, n, nclasses, 1 if n > 1000 else R.INEXACT_QUOTA):
                pick, cnt, out = _run(F, c["rows"], 1, n, n, [n], method, c["params"], log_domain, c["cls"])
                k = int(cnt[0])
                tag = "%s/%d n=%d classes=%d seed %d" % (R.METHODS[method], log_domain, n, nclasses, c["seed_index"])
                assert k == len(c["pick"]) and np.array_equal(pick[0, :k], c["pick"]), "%s: picks" % tag
                assert np.all(pick[0, k:] == SENT)
                got = out[0][c["pick"] - 1].astype(np.float64)
                err = np.abs(got - c["scores"])
                if not log_domain:
                    err = err / np.maximum(np.abs(c["scores"]), np.finfo(np.float64).tiny)
                e = float(err.max()) if k else 0.0
                print("%s: error %.3g, bound %.3g, margin %.3g" % (tag, e, c["bound"], c["stats"]["margin"]))
                assert e <= c["bound"], "%s: score error %.3g above the bound %.3g" % (tag, e, c["bound"])
                worst = max(worst, e / c["bound"])
    print("largest error / bound: %.3f" % worst)


# ------------------------------------------------------------------------------------------------ Detector level
H, W = 128, 176
SEEDS = list(range(5, 13))
SOFT = dict(gaussian=dict(method="gaussian"), linear=dict(method="linear"))


@pytest.fixture(scope="module")
def setup(F):
    import torch
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    weights.copy_(torch.from_numpy(_amplified_weights(model["native"], w, 17, cls_gain=200.0)))
    frames = _frames(F, SEEDS, H, W)
    s = dict(cfg=cfg, model=model, weights=weights, gradient=gradient, frames=frames)
    s["plain"] = _collect(F.Detector(model), frames)
    for name, t in SOFT.items():
        s[name] = _soft_collect(F, F.Detector(model, nms=t), frames)
    # what the tests below lean on: two class-test survivors of one class that overlap by more than 0.1 in some frame
    pairs = 0
    for r in s["gaussian"]:
        if "bb" not in r:
            continue
        bb, kc = r["bb"].astype(np.float64), r["kc"]
        area = (bb[:, 2] - bb[:, 0] + 1) * (bb[:, 3] - bb[:, 1] + 1)
        for a in range(len(kc)):
            w = np.maximum(0, np.minimum(bb[:, 2], bb[a, 2]) - np.maximum(bb[:, 0], bb[a, 0]) + 1)
            h = np.maximum(0, np.minimum(bb[:, 3], bb[a, 3]) - np.maximum(bb[:, 1], bb[a, 1]) + 1)
            iou = w * h / (area + area[a] - w * h)
            pairs += int(np.sum((iou[a + 1:] > 0.1) & (kc[a + 1:] == kc[a])))
    print("soft nms: survivors %s, winners plain %s gaussian %s linear %s, overlapping same-class pairs %d"
          % ([r["kept"] for r in s["plain"]], [r["nwin"] for r in s["plain"]], [r["nwin"] for r in s["gaussian"]],
             [r["nwin"] for r in s["linear"]], pairs))
    assert pairs > 0, "no frame has two survivors of one class that overlap: nothing is exercised"
    assert any(g["nwin"] > p["nwin"] for g, p in zip(s["gaussian"], s["plain"])), "the soft pass keeps no box the hard cut deletes"
    return s


def _soft_collect(F, d, frames):
    """_collect, plus the record's bb / kc and the frame's keep_row and r2 rows (the Detector's own buffers), per frame"""
    out = []
    for f in frames:
        r = _collect(d, [f])[0]
        rec = d._last
        R_ = len(r["pick"])
        if "bb" in rec:
            r.update(bb=rec["bb"].copy(), kc=rec["kc"].copy(), keep_row=d._buf("keep_row", (R_,), np.int32).numpy()[:r["kept"]],
                     r2=d._buf("r2", (R_, 4), np.float64).numpy()[:r["kept"]])
        out.append(r)
    return out


def _winner_keys(winners):
    """(class, candidate, confidence, r2) of _winner_rows' tuples"""
    return [(w[0], w[4], w[1], w[9:13]) for w in winners]


def test_setting_off_changes_nothing_and_launches_nothing_new(F, setup):
    s = setup
    got = {}

    def run(name, d):
        def fn():
            got[name] = _collect(d, s["frames"])
            got[name + "/batch"] = d.detect_batch(s["frames"])
            got[name + "/records"] = d.last_batch
        return _launches(F, fn)
    la0 = run("absent", F.Detector(s["model"]))
    la1 = run("hard", F.Detector(s["model"], nms=dict(method="hard")))
    la2 = run("empty", F.Detector(s["model"], nms={}))
    assert la0["soft_nms"] == 0 and la0 == la1 == la2, "the same launches per kernel class"
    for name in ("absent", "hard", "empty"):
        _same(got[name], s["plain"], name)
        for b in range(len(SEEDS)):
            assert _winner_rows(got[name + "/batch"][b]) == s["plain"][b]["winners"], (name, b)
            assert "bb" not in got[name + "/records"][b] and "kc" not in got[name + "/records"][b]
    la3 = _launches(F, lambda: _collect(F.Detector(s["model"], nms=dict(method="gaussian")), s["frames"]))
    busy = sum(r["n"] > 0 and len(r["pick"]) > 0 for r in s["plain"])
    assert la3["soft_nms"] == busy > 0 and la3["nms"] < la0["nms"]


def _expected(r, pick):
    """the winners of a frame from the restatement's picks on its record: classes ascending, pick order within a class ->
    [(class, candidate, position in pick)]"""
    kc = r["kc"]
    want = []
    for c in sorted(set(kc[pick - 1].tolist())):
        for q in np.nonzero(kc[pick - 1] == c)[0]:
            want.append((int(c), int(r["keep_row"][pick[q] - 1]) + 1, int(q)))
    return want


def test_gaussian_winners_are_the_fp32_restatements_on_the_record(F, setup):
    s = setup
    deep = 0
    for b, r in enumerate(s["gaussian"]):
        if "bb" not in r:
            assert r["nwin"] == 0
            continue
        pick, sc = R.soft_nms_f32(r["bb"], 5, R.GAUSSIAN, 0.1, 0.5, LOG_MIN, 1, r["kc"])
        want = _expected(r, pick)
        got = _winner_keys(r["winners"])
        assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want], "frame %d: class, candidate, order" % b
        for g, w in zip(got, want):
            assert np.float32(g[2]).view(np.uint32) == sc[w[2]].view(np.uint32), "frame %d: confidence" % b
            assert g[3] == tuple(r["r2"][pick[w[2]] - 1].tolist()), "frame %d: r2" % b
        deep += len(want) > s["plain"][b]["nwin"]
    assert deep > 0


def test_linear_winners_are_the_float64_restatements_on_the_record(F, setup):
    """log1pf is inexact: frames whose float64 margin exceeds twice the bound (general coordinates: IOU_ERR_GENERAL)"""
    s = setup
    checked = 0
    for b, r in enumerate(s["linear"]):
        if "bb" not in r or r["kept"] == 0:
            continue
        bb = r["bb"]
        assert np.all(np.isfinite(bb[:, :4])) and np.all(bb[:, 2] >= bb[:, 0]) and np.all(bb[:, 3] >= bb[:, 1]), "the bound's precondition"
        pick, sc, st = R.soft_nms_f64(bb, 5, R.LINEAR, 0.1, 0.5, LOG_MIN, 1, r["kc"])
        bound = R.score_error_bound(R.LINEAR, 1, 0.5, st, R.IOU_ERR_GENERAL)
        print("frame %d: margin %.3g, bound %.3g, decays %d" % (b, st["margin"], bound, st["decays"]))
        if not st["margin"] > 2.0 * bound:
            continue
        checked += 1
        want = _expected(r, pick)
        got = _winner_keys(r["winners"])
        assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want], "frame %d: class, candidate, order" % b
        for g, w in zip(got, want):
            assert abs(g[2] - sc[w[2]]) <= bound, "frame %d: confidence" % b
            assert g[3] == tuple(r["r2"][pick[w[2]] - 1].tolist()), "frame %d: r2" % b
    assert checked >= len(SEEDS) // 2, "more than half of the frames fail the margin rule (%d checked)" % checked


def test_confidence_is_the_decayed_score(F, setup):
    s = setup
    lowered = 0
    for b, r in enumerate(s["gaussian"]):
        seen = set()
        for cls, cand, conf, _ in _winner_keys(r["winners"]):
            raw = r["cnet"]["cls"][cand - 1, cls - 1]
            if cls not in seen:     # the first winner of a class was never decayed
                assert np.float32(conf).view(np.uint32) == raw.view(np.uint32), "frame %d class %d" % (b, cls)
                seen.add(cls)
            else:
                assert conf <= float(raw), "frame %d class %d" % (b, cls)
                lowered += conf < float(raw)
    assert lowered > 0


def test_min_score_zero_returns_every_survivor(F, setup):
    s = setup
    for name in SOFT:
        d = F.Detector(s["model"], nms=dict(SOFT[name], min_score=0))
        some = 0
        for f in s["frames"]:
            win = d.detect(f)
            assert len(win) == d._last["kept"]
            some += len(win)
        assert some > 0


@pytest.mark.parametrize("name", sorted(SOFT))
def test_detect_batch_equals_the_detect_loop_under_a_soft_method(F, setup, name):
    s = setup
    props = dict(order="score", pre_nms_top_n=50)
    want = _soft_collect(F, F.Detector(s["model"], nms=SOFT[name], proposals=props), s["frames"])
    assert any(r["nwin"] > 0 for r in want)
    for batch in (8, 3):
        d = F.Detector(s["model"], nms=SOFT[name], proposals=props)
        d.BATCH = batch
        res = d.detect_batch(s["frames"])
        for b, (rec, win, w) in enumerate(zip(d.last_batch, res, want)):
            tag = "%s BATCH %d frame %d" % (name, batch, b)
            assert _winner_rows(win) == w["winners"], tag
            assert rec["n"] == w["n"] and rec["kept"] == w["kept"] and np.array_equal(rec["pick"], w["pick"]), tag
            for k in ("bbox", "cls"):
                assert (rec["cnet"] is None) == (w["cnet"] is None)
                if w["cnet"] is not None:
                    assert np.array_equal(rec["cnet"][k], w["cnet"][k]), tag
            if "bb" in w:
                assert np.array_equal(rec["bb"].view(np.uint32), w["bb"].view(np.uint32)) and np.array_equal(rec["kc"], w["kc"]), tag
    # shared_cnet keeps working under the setting
    d = F.Detector(s["model"], nms=SOFT[name], proposals=props)
    res = d.detect_batch(s["frames"], shared_cnet=True)
    assert sum(len(x) for x in res) > 0


def test_evaluate_detections_in_batches_under_gaussian(F, setup):
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import evaluate_detections
    s = setup
    d = F.Detector(s["model"], nms=SOFT["gaussian"])
    items = []
    for img in s["frames"][:6]:
        rois = []
        for j, x in enumerate(list(d.detect(img))[::3]):
            r = x["r2"]
            rois.append(F.Roi(Rect(r.minX, r.minY, r.maxX, r.maxY) if j % 2 == 0 else r.offset(r.width() * 0.8, 0), x["class"]))
        rois.append(F.Roi(Rect(5, 5, 40, 40), 16))
        items.append(dict(img=img, rois=rois))
    one = evaluate_detections(F.Detector(s["model"], nms=SOFT["gaussian"]), _Val(items), len(items), batch=1)
    assert one["detections"] > 0 and one["tp"] > 0
    four = evaluate_detections(F.Detector(s["model"], nms=SOFT["gaussian"]), _Val(items), len(items), batch=4)
    assert four == one


def test_hard_with_an_overlap_of_its_own(F, setup):
    """"hard" at 0.3: the winners are nms() per class at 0.3 on the record of a soft run of the same frame -- the class test's
    survivors do not depend on the setting"""
    s = setup
    d = F.Detector(s["model"], nms=dict(method="hard", overlap=0.3))
    la = _launches(F, lambda: d.detect(s["frames"][0]))
    assert la["soft_nms"] == 0
    for b, f in enumerate(s["frames"]):
        r = s["gaussian"][b]
        win = d.detect(f)
        assert d._last["kept"] == r["kept"] and "bb" not in d._last
        if "bb" not in r:
            assert len(win) == 0
            continue
        want = []
        for c in sorted(set(r["kc"].tolist())):
            rows = np.nonzero(r["kc"] == c)[0]
            for i in F.nms(r["bb"][rows], 0.3).tolist():
                want.append((int(c), int(r["keep_row"][rows[i - 1]]) + 1))
        assert [(x["class"], x["candidate"]) for x in win] == want, "frame %d" % b
        for x in win:        # a hard winner's confidence is the undecayed one
            assert np.float32(x["confidence"]).view(np.uint32) == r["cnet"]["cls"][x["candidate"] - 1, x["class"] - 1].view(np.uint32)
