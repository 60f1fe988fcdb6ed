"""Test-time augmentation on the device (cfg.tta, frcnn_detect_merge_views).  Kernel level, against the restatement of
tests/tta_ref.py: every output bit for bit, nothing stored behind a frame's K' rows or behind its candidates, a frame's result
independent of its neighbours, argument errors without a launch.  Detector level (the fixture of test_gpu_box_vote.py: vgg_small,
amplified weights, 128x176 frames): the key absent or an identity table changes nothing and launches nothing new; with the key the
Detector's views are the test's own (numpy mirror, frcnn_image_scale), and its result is what a plain Detector finds on those
views, merged by the restatement and cut per class by nms() -- winners, order, classes, confidences, view, candidate and r2 bit for
bit; chunking, voting and Soft-NMS across views, evaluate_detections in batches."""
import ctypes as C

import numpy as np
import pytest

import box_vote_ref as V
import detect_classes_ref as D
import soft_nms_ref as S
import tta_ref as T
from test_gpu_detect_batch import _Val, _amplified_weights, _frames, _winner_rows
from test_gpu_proposals import _collect, _launches, _same
from test_gpu_soft_nms import H, SEEDS, W

pytestmark = pytest.mark.gpu
SENT = -7
GUARD = 8
# (flip, Wv, ax, ay) of up to 8 views of a 128 x 176 frame: the frame, its mirror, scales 1.3 (166 x 228: neither factor is a short
# fraction, ax != ay), 1.25 (176 / 220 = 128 / 160 = 0.8) and 0.5, each with its mirror
GEO = [(0, 176.0, 1.0, 1.0), (1, 176.0, 1.0, 1.0), (0, 228.0, 176.0 / 228, 128.0 / 166), (1, 228.0, 176.0 / 228, 128.0 / 166),
       (0, 220.0, 176.0 / 220, 128.0 / 160), (1, 220.0, 176.0 / 220, 128.0 / 160), (0, 88.0, 2.0, 2.0), (1, 88.0, 2.0, 2.0)]


# ------------------------------------------------------------------------------------------------ kernel level
def _problem(seed, nF, nV, rs, ms, first=0):
    """Synthetic segments of nF frames of nV views.  Segment i (counted from `first`) has K = rs, 0 or a random count -- one in
    three above rs, which the kernel clips -- and R = a random count, ms or 0, so that every call of three segments or more has a
    view without survivors, a full one and one without candidates.  Mirrored views hold rects that touch 0 and Wv."""
    rng = np.random.RandomState(seed)
    Sg = nF * nV
    geo = [GEO[(v + (f if nV == 1 else 0)) % 8] for f in range(nF) for v in range(nV)]
    K = [[rs, 0, int(rng.randint(0, rs + 1))][(first + i) % 3] for i in range(Sg)]
    Kdev = [k + 5 if (first + i) % 3 == 0 and i % 2 else k for i, k in enumerate(K)]      # (a count above the stride is clipped)
    R = [[int(rng.randint(0, ms + 1)), ms, 0][(first + i) % 3] for i in range(Sg)]
    bb = rng.standard_normal((Sg * rs, 5)).astype(np.float32)
    kc = rng.randint(1, 17, Sg * rs).astype(np.int32)
    keep = np.concatenate([rng.randint(0, max(R[i], 1), rs) for i in range(Sg)]).astype(np.int32) if rs else np.zeros(0, np.int32)
    r2 = np.empty((Sg * rs, 4), np.float64)
    for i in range(Sg):
        Wv = geo[i][1]
        x1 = rng.uniform(-3.0, Wv - 4.0, rs); y1 = rng.uniform(-3.0, 120.0, rs)
        seg = np.stack([x1, y1, x1 + rng.uniform(1.0, 60.0, rs), y1 + rng.uniform(1.0, 60.0, rs)], 1)
        seg[0::5, 0] = 0.0            # rects that touch the view's left and right edge
        seg[1::5, 2] = Wv
        seg[2::7] = np.round(seg[2::7])
        r2[i * rs:(i + 1) * rs] = seg
    counts = rng.randint(0, 5000, (4, Sg)).astype(np.int32)
    counts[2] = Kdev
    pick = rng.randint(1, ms + 1, Sg * ms).astype(np.int64) if ms else np.zeros(0, np.int64)
    return dict(F=nF, V=nV, rs=rs, ms=ms, geo=geo, K=K, R=R, bb=bb, kc=kc, keep_row=keep, r2=r2, counts=counts, pick=pick)


def _run(F, p):
    """frcnn_detect_merge_views on a _problem -> the outputs with their guard tails; asserts that the inputs come back unchanged"""
    nF, nV, rs, ms = p["F"], p["V"], p["rs"], p["ms"]
    Sg = nF * nV
    dev = dict((k, F.DeviceTensor.from_numpy(p[k])) for k in ("bb", "kc", "keep_row", "r2", "counts", "pick"))
    out = dict(bb=np.full((Sg * rs + GUARD, 5), SENT, np.float32), kc=np.full(Sg * rs + GUARD, SENT, np.int32),
               keep_row=np.full(Sg * rs + GUARD, SENT, np.int32), r2=np.full((Sg * rs + GUARD, 4), SENT, np.float64),
               pick=np.full(Sg * ms + GUARD, SENT, np.int64), counts=np.full(4 * nF + GUARD, SENT, np.int32))
    o = dict((k, F.DeviceTensor.from_numpy(a)) for k, a in out.items())
    geo = p["geo"]
    F._lib.call("frcnn_detect_merge_views", F.ptr(dev["bb"]), F.ptr(dev["kc"]), F.ptr(dev["keep_row"]), F.ptr(dev["r2"]), rs,
                F.ptr(dev["counts"]), F.ptr(dev["pick"]), ms, nF, nV, (C.c_int * Sg)(*[g[0] for g in geo]),
                (C.c_double * Sg)(*[g[1] for g in geo]), (C.c_double * Sg)(*[g[2] for g in geo]),
                (C.c_double * Sg)(*[g[3] for g in geo]), (C.c_int * Sg)(*p["R"]), F.ptr(o["bb"]), F.ptr(o["kc"]),
                F.ptr(o["keep_row"]), F.ptr(o["r2"]), F.ptr(o["pick"]), F.ptr(o["counts"]), F.stream_ptr())
    for k in dev:
        assert dev[k].numpy().tobytes() == p[k].tobytes(), "input %s was written" % k
    return dict((k, t.numpy()) for k, t in o.items())


def _want(p):
    """the restatement's outputs, laid out as the kernel's: sentinels wherever nothing may be stored"""
    nF, nV, rs, ms = p["F"], p["V"], p["rs"], p["ms"]
    Sg = nF * nV
    want = dict(bb=np.full((Sg * rs + GUARD, 5), SENT, np.float32), kc=np.full(Sg * rs + GUARD, SENT, np.int32),
                keep_row=np.full(Sg * rs + GUARD, SENT, np.int32), r2=np.full((Sg * rs + GUARD, 4), SENT, np.float64),
                pick=np.full(Sg * ms + GUARD, SENT, np.int64), counts=np.full(4 * nF + GUARD, SENT, np.int32))
    for f in range(nF):
        rows = []
        for v in range(nV):
            i = f * nV + v
            a, k = i * rs, p["K"][i]
            rows.append(dict(bb=p["bb"][a:a + k], kc=p["kc"][a:a + k], keep_row=p["keep_row"][a:a + k], r2=p["r2"][a:a + k],
                             pick=p["pick"][i * ms:i * ms + p["R"][i]], n=p["counts"][0, i]))
        m = T.merge(rows, p["geo"][f * nV:(f + 1) * nV], ms)
        a, k = f * nV * rs, m["counts"][2]
        for name in ("bb", "kc", "keep_row", "r2"):
            want[name][a:a + k] = m[name]
        want["pick"][f * nV * ms:f * nV * ms + m["counts"][1]] = m["pick"]
        for q in range(3):
            want["counts"][q * nF + f] = m["counts"][q]
    return want


def _compare(got, want, tag):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), "%s: %s differs from the restatement" % (tag, k)


@pytest.mark.parametrize("nV", [1, 2, 3, 8])
@pytest.mark.parametrize("rs", [1, 63, 65, 700])
def test_merge_against_the_restatement(F, rs, nV):
    seen = set()
    for nF in (1, 3):
        for ms in (max(rs // 2, 1), rs + 9):
            p = _problem(1000 * rs + 10 * nV + nF, nF, nV, rs, ms, first=nF + ms)
            _compare(_run(F, p), _want(p), "F %d V %d rows %d match rows %d" % (nF, nV, rs, ms))
            for i in range(nF * nV):
                seen |= {("K", "none" if p["K"][i] == 0 else "full" if p["K"][i] == rs else "some"),
                         ("R", "none" if p["R"][i] == 0 else "some"), ("flip", p["geo"][i][0]),
                         ("ax != ay", p["geo"][i][2] != p["geo"][i][3])}
    assert {("K", "none"), ("K", "full"), ("R", "none"), ("R", "some"), ("flip", 1), ("flip", 0)} <= seen, seen
    assert nV < 3 or ("ax != ay", True) in seen


def test_mirrored_rects_that_touch_the_edges_and_an_identity_view_by_hand(F):
    """one frame, three views of one survivor each: the frame (bits kept, -0.0 included), its mirror (0 and Wv swap exactly),
    a mirrored 1.3 view (ax != ay)"""
    p = _problem(1, 1, 3, 1, 2)
    p["geo"] = [GEO[0], GEO[1], GEO[3]]
    p["K"], p["R"] = [1, 1, 1], [2, 0, 1]
    p["counts"][2] = [1, 1, 1]
    p["r2"][:] = [[-0.0, 3.0, 176.0, 7.5], [0.0, 3.0, 176.0, 7.5], [0.0, 16.6, 228.0, 83.0]]
    p["keep_row"][:] = [1, 0, 0]
    got = _run(F, p)
    _compare(got, _want(p), "by hand")
    assert got["r2"][0].tobytes() == p["r2"][0].tobytes() and got["r2"][1].tolist() == [0.0, 3.0, 176.0, 7.5]
    assert got["r2"][2].tolist() == [0.0, 16.6 * (128.0 / 166), 228.0 * (176.0 / 228), 83.0 * (128.0 / 166)]
    assert got["keep_row"][:3].tolist() == [1, 2, 2] and got["pick"][:3].tolist() == [p["pick"][0], p["pick"][1], 4 + p["pick"][4]]


def test_a_frame_does_not_depend_on_its_neighbours_or_on_the_frame_count(F):
    nV, rs, ms = 3, 65, 40
    alone = _problem(7, 1, nV, rs, ms)
    three = _problem(8, 3, nV, rs, ms)
    for k in ("bb", "kc", "keep_row", "r2"):       # frame 2 of the call of three is the frame of the call of one
        three[k][2 * nV * rs:] = alone[k]
    three["pick"][2 * nV * ms:] = alone["pick"]
    three["counts"][:, 2 * nV:] = alone["counts"]
    three["K"][2 * nV:], three["R"][2 * nV:], three["geo"][2 * nV:] = alone["K"], alone["R"], alone["geo"]
    a, b = _run(F, alone), _run(F, three)
    _compare(a, _want(alone), "alone")
    _compare(b, _want(three), "among three")
    for k in ("bb", "kc", "keep_row", "r2"):
        assert a[k][:nV * rs].tobytes() == b[k][2 * nV * rs:3 * nV * rs].tobytes(), k
    assert a["pick"][:nV * ms].tobytes() == b["pick"][2 * nV * ms:3 * nV * ms].tobytes()
    assert [a["counts"][q] for q in range(3)] == [b["counts"][3 * q + 2] for q in range(3)]
    assert sum(alone["K"]) > 0 and sum(alone["R"]) > 0


def test_argument_errors_launch_nothing_and_store_nothing(F):
    nF, nV, rs, ms = 2, 2, 16, 16
    p = _problem(3, nF, nV, rs, ms)
    Sg = nF * nV
    dev = dict((k, F.DeviceTensor.from_numpy(p[k])) for k in ("bb", "kc", "keep_row", "r2", "counts", "pick"))
    outs = dict(bb_out=np.full((Sg * rs, 5), SENT, np.float32), kc_out=np.full(Sg * rs, SENT, np.int32),
                keep_row_out=np.full(Sg * rs, SENT, np.int32), r2_out=np.full((Sg * rs, 4), SENT, np.float64),
                pick_out=np.full(Sg * ms, SENT, np.int64), counts_out=np.full(4 * nF, SENT, np.int32))
    o = dict((k, F.DeviceTensor.from_numpy(a)) for k, a in outs.items())
    ints = lambda v: (C.c_int * len(v))(*v)
    dbl = lambda v: (C.c_double * len(v))(*v)
    geo = p["geo"]
    good = dict(bb=F.ptr(dev["bb"]), kc=F.ptr(dev["kc"]), keep_row=F.ptr(dev["keep_row"]), r2=F.ptr(dev["r2"]), row_stride=rs,
                counts=F.ptr(dev["counts"]), pick=F.ptr(dev["pick"]), match_stride=ms, F=nF, V=nV, flip=ints([g[0] for g in geo]),
                wv=dbl([g[1] for g in geo]), ax=dbl([g[2] for g in geo]), ay=dbl([g[3] for g in geo]), R=ints(p["R"]))
    good.update((k, F.ptr(t)) for k, t in o.items())
    nan, inf = float("nan"), float("inf")
    bad = [dict(F=0), dict(F=-1), dict(F=65536), dict(V=0), dict(V=9), dict(V=-2), dict(row_stride=-1), dict(match_stride=-1),
           dict(flip=None), dict(wv=None), dict(ax=None), dict(ay=None), dict(R=None), dict(counts=None), dict(counts_out=None),
           dict(bb=None), dict(kc=None), dict(keep_row=None), dict(r2=None), dict(pick=None), dict(bb_out=None), dict(kc_out=None),
           dict(keep_row_out=None), dict(r2_out=None), dict(pick_out=None),
           dict(wv=dbl([176.0, 0.0, 176.0, 176.0])), dict(wv=dbl([176.0, 176.0, -1.0, 176.0])), dict(wv=dbl([nan] * 4)),
           dict(wv=dbl([inf] * 4)), dict(ax=dbl([1.0, 1.0, 1.0, 0.0])), dict(ax=dbl([1.0, nan, 1.0, 1.0])),
           dict(ax=dbl([1.0, 1.0, inf, 1.0])), dict(ay=dbl([-0.5, 1.0, 1.0, 1.0])), dict(ay=dbl([1.0, 1.0, 1.0, nan])),
           dict(ay=dbl([inf, 1.0, 1.0, 1.0])), dict(R=ints([0, 0, 0, ms + 1])), dict(R=ints([-1, 0, 0, 0]))]

    def call(args):
        F._lib.call("frcnn_detect_merge_views", *(list(args.values()) + [F.stream_ptr()]))

    def errors():
        for t in bad:
            with pytest.raises(F.FrcnnError):
                call(dict(good, **t))
    la = _launches(F, errors)
    assert sum(la.values()) == 0, la
    for k, t in o.items():
        assert np.all(t.numpy() == SENT), "an argument error stored something in %s" % k
    la = _launches(F, lambda: call(good))
    assert la["elemwise"] == 1 and sum(la.values()) == 1, la          # one launch, counted under elemwise
    assert o["counts_out"].numpy()[2 * nF:3 * nF].tolist() == [p["K"][0] + p["K"][1], p["K"][2] + p["K"][3]]


# ------------------------------------------------------------------------------------------------ Detector level
NF = 5                      # frames of the fixture
FLIP = dict(hflip=True)
SCALES = dict(scales=[1, 1.25])
BOTH = dict(hflip=True, scales=[1, 1.25])
VOTE = dict(overlap=0.1)    # (test_gpu_box_vote.py: whatever the per-class pass deletes votes for a winner)


def _keys(win):
    """what identifies a winner and where it is: (class, confidence as fp32, candidate, view, r2 x 4)"""
    return [(x["class"], float(np.float32(x["confidence"])), x["candidate"], x["view"], x["r2"].minX, x["r2"].minY, x["r2"].maxX,
             x["r2"].maxY) for x in win]


_REC = ("bb", "kc", "r2", "keep_row", "pick", "votes")


def _frame_state(win, rec):
    """everything a frame leaves behind under the key"""
    out = dict(keys=_keys(win), rows=[w + (x["view"],) for w, x in zip(_winner_rows(win), win)], n=rec["n"], kept=rec["kept"],
               roff=rec["roff"].tolist(), nviews=len(rec["views"]))
    for k in _REC:
        if k in rec:
            out[k] = rec[k].copy()
    out["views"] = [dict(n=r["n"], kept=r["kept"], pick=r["pick"].copy(), p=r["p"].copy(), rect=r["rect"].copy(),
                         cls=None if r["cnet"] is None else r["cnet"]["cls"].copy()) for r in rec["views"]]
    return out


def _same_state(a, b, tag):
    assert a["keys"] == b["keys"] and a["rows"] == b["rows"], tag
    assert (a["n"], a["kept"], a["roff"], a["nviews"]) == (b["n"], b["kept"], b["roff"], b["nviews"]), tag
    for k in _REC:
        assert (k in a) == (k in b), (tag, k)
        if k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    for v, (x, y) in enumerate(zip(a["views"], b["views"])):
        assert (x["n"], x["kept"]) == (y["n"], y["kept"]), (tag, v)
        for k in ("pick", "p", "rect", "cls"):
            assert (x[k] is None) == (y[k] is None) and (x[k] is None or x[k].tobytes() == y[k].tobytes()), (tag, v, k)


def _tta_collect(F, d, frames):
    return [_frame_state(d.detect(f), d._last) for f in frames]


@pytest.fixture(scope="module")
def setup(F):
    import torch
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    weights.copy_(torch.from_numpy(_amplified_weights(model["native"], w, 17, cls_gain=200.0)))
    frames = _frames(F, SEEDS[:NF], H, W)
    s = dict(cfg=cfg, model=model, weights=weights, gradient=gradient, frames=frames)
    s["plain"] = _collect(F.Detector(model), frames)
    return s


def test_key_absent_and_identity_tables_change_nothing_and_launch_nothing_new(F, setup):
    s = setup
    got, las = {}, {}

    def run(name, d):
        def fn():
            got[name] = _collect(d, s["frames"])
            got[name + "/batch"] = d.detect_batch(s["frames"])
            got[name + "/records"] = d.last_batch
        las[name] = _launches(F, fn)
        assert not [k for k in d._bufs if "tta" in k], "%s: nothing new is allocated" % name
    run("plain", F.Detector(s["model"]))
    run("none", F.Detector(s["model"], tta=None))
    run("empty", F.Detector(s["model"], tta={}))
    run("one", F.Detector(s["model"], tta=dict(scales=[1.0], hflip=False)))
    run("cfg", F.Detector(dict(s["model"], cfg=dict(s["cfg"], tta=dict(scales=[1])))))
    want_rec = got["plain/records"]
    for name in ("plain", "none", "empty", "one", "cfg"):
        assert las[name] == las["plain"], "%s: the same launches per kernel class" % name
        _same(got[name], s["plain"], name)
        for b in range(NF):
            assert _winner_rows(got[name + "/batch"][b]) == s["plain"][b]["winners"], (name, b)
            rec = got[name + "/records"][b]
            assert "views" not in rec and "bb" not in rec and rec.keys() == want_rec[b].keys(), (name, b)
            assert all("view" not in x for x in got[name + "/batch"][b])
    # the cfg's key is read when the call names none, and the call's table wins
    m = dict(s["model"], cfg=dict(s["cfg"], tta=dict(hflip=True)))
    assert F.Detector(m).tta == (True, (1.0,)) and F.Detector(m, tta=dict(scales=[2])).tta == (False, (2.0,))
    # proposals() does not look at the key
    a, b = F.Detector(s["model"]).proposals(s["frames"][0]), F.Detector(s["model"], tta=BOTH).proposals(s["frames"][0])
    assert len(a) == len(b) > 0 and [(x["p"], x["l"]) for x in a] == [(x["p"], x["l"]) for x in b]


def _test_views(F, x, view_list):
    """the test's own views of frame x: numpy mirror, frcnn_image_scale"""
    out = []
    for sc, flip, dH, dW in view_list:
        if not flip:
            base = x
            if sc != 1.0:
                d = F.DeviceTensor.from_numpy(x)
                o = F.DeviceTensor.empty((3, dH, dW)); tmp = F.DeviceTensor.empty((3 * H * dW,))
                F._lib.call("frcnn_image_scale", F.ptr(d), 3, H, W, F.ptr(o), dH, dW, F.ptr(tmp), 0, F.stream_ptr())
                base = o.numpy()
        out.append(np.ascontiguousarray(base[:, :, ::-1]) if flip else base)
    return out


def _survivors(d, view, ncls):
    """what the class test of a plain Detector d leaves of one view, from its record (d votes, only for the record to keep its
    rows; the record's r2 is the unvoted one): checked against the restatement of the class test"""
    d.detect(view)
    rec = d._last
    rec["p"], rec["rect"]         # (fetched now: the record views buffers that d's next frame overwrites)
    if rec["n"] == 0 or len(rec["pick"]) == 0:
        return dict(bb=np.zeros((0, 5), np.float32), kc=np.zeros(0, np.int32), keep_row=np.zeros(0, np.int32),
                    r2=np.zeros((0, 4)), pick=np.zeros(0, np.int64), n=rec["n"]), rec
    ref = D.detect_classes(rec["cnet"]["cls"], ncls, 0.2, D.TOP)
    assert np.array_equal(ref["cand"], rec["keep_row"]) and np.array_equal(ref["cls"], rec["kc"])
    assert np.array_equal(ref["conf"], rec["bb"][:, 4]) and np.array_equal(rec["bb"][:, :4], rec["r2"].astype(np.float32))
    return dict(bb=rec["bb"], kc=rec["kc"], keep_row=rec["keep_row"], r2=rec["r2"], pick=rec["pick"], n=rec["n"]), rec


def _check_against_plain_views(F, s, tta):
    model, ncls = s["model"], s["cfg"]["class_count"] + 1
    hflip, scales = tta.get("hflip", False), tta.get("scales", [1.0])
    d = F.Detector(model, tta=tta)
    plain = F.Detector(model, box_voting=dict(overlap=1.0))
    total = cross = 0
    for b, x in enumerate(s["frames"]):
        tag = "%r frame %d" % (tta, b)
        vl = T.views(hflip, scales, H, W)
        win = d.detect(x)
        rec = d._last
        views = _test_views(F, x, vl)
        for i, (v, (sc, flip, dH, dW)) in enumerate(zip(views, vl)):
            if flip or sc != 1.0:     # the Detector's view, bit for bit
                assert d._buf("tta_view_0_%d" % i, (3, dH, dW)).numpy().tobytes() == v.tobytes(), (tag, i)
        rows, recs = zip(*[_survivors(plain, v, ncls) for v in views])
        cap = max(d._layout_of(dH, dW).anchors for _, _, dH, dW in vl)
        m = T.merge(rows, T.geometry(vl, H, W), cap)
        assert (rec["n"], rec["kept"]) == (m["counts"][0], m["counts"][2]) and rec["roff"].tolist() == m["roff"].tolist(), tag
        for k in ("bb", "kc", "keep_row", "r2", "pick"):
            assert rec[k].dtype == m[k].dtype and rec[k].tobytes() == m[k].tobytes(), (tag, k)
        for v, (vr, pr) in enumerate(zip(rec["views"], recs)):      # a view's record is the plain Detector's record of the view
            assert vr["n"] == pr["n"] and vr["kept"] == pr["kept"] and np.array_equal(vr["pick"], pr["pick"]), (tag, v)
            assert vr["p"].tobytes() == pr["p"].tobytes() and vr["rect"].tobytes() == pr["rect"].tobytes(), (tag, v)
        # the per-class pass: classes ascending, per class nms() over the merged rows of that class, in their order
        want = []
        for c in sorted(set(m["kc"].tolist())):
            idx = np.nonzero(m["kc"] == c)[0]
            for j in idx[F.nms(m["bb"][idx], 0.1) - 1].tolist():
                cand = int(m["keep_row"][j]) + 1
                want.append((c, float(m["bb"][j, 4]), cand, T.view_of(cand, m["roff"])) + tuple(m["r2"][j].tolist()))
        assert _keys(win) == want, tag
        for x_, w in zip(win, want):       # p, r and a describe the anchor in the view's coordinates
            pr = recs[w[3]]
            i = int(pr["pick"][w[2] - 1 - int(m["roff"][w[3]])]) - 1
            assert np.float32(x_["p"]) == pr["p"][i] and [x_["r"].minX, x_["r"].minY, x_["r"].maxX, x_["r"].maxY] == pr["rect"][i].tolist()
        total += len(want)
        cross += len(set(w[3] for w in want)) > 1
    print("%r: %d winners, %d frames whose winners come from more than one view" % (tta, total, cross))
    assert total > 0 and (cross > 0 or len(vl) == 1), "no frame has winners of two views: the merge decides nothing"


def test_hflip_equals_a_plain_detector_on_the_frame_and_its_numpy_mirror(F, setup):
    _check_against_plain_views(F, setup, FLIP)


@pytest.mark.parametrize("tta", [SCALES, BOTH, dict(scales=[1.25])], ids=["scales", "both", "one scaled view"])
def test_scales_and_both_equal_a_plain_detector_on_the_views(F, setup, tta):
    _check_against_plain_views(F, setup, tta)


@pytest.mark.parametrize("batch", [8, 2])
def test_detect_batch_chunks_equal_the_detect_loop(F, setup, batch):
    s = setup
    want = _tta_collect(F, F.Detector(s["model"], tta=FLIP), s["frames"])
    assert sum(len(w["keys"]) for w in want) > 0
    d = F.Detector(s["model"], tta=FLIP)
    d.BATCH = batch                     # V = 2: chunks of 4 + 1 frames, or of one
    res = d.detect_batch(s["frames"])
    assert len(res) == len(d.last_batch) == NF
    for b in range(NF):                 # (the records of every chunk but the last are detached copies)
        _same_state(_frame_state(res[b], d.last_batch[b]), want[b], "BATCH %d frame %d" % (batch, b))


def _winner_rows_of(st):
    """the merged row (0-based) of every winner: keep_row is the survivors' candidate position, unique under the top-class test"""
    pos = dict((int(c) + 1, j) for j, c in enumerate(st["keep_row"].tolist()))
    return np.array([pos[k[2]] for k in st["keys"]], np.int64)


def test_voting_across_views(F, setup):
    s = setup
    plain = _tta_collect(F, F.Detector(s["model"], tta=BOTH), s["frames"])
    voted = _tta_collect(F, F.Detector(s["model"], tta=BOTH, box_voting=VOTE), s["frames"])
    crossed = moved = 0
    for b, (v, p) in enumerate(zip(voted, plain)):
        tag = "frame %d" % b
        assert [k[:4] for k in v["keys"]] == [k[:4] for k in p["keys"]], "%s: who wins does not change" % tag
        for k in ("bb", "kc", "r2", "keep_row", "pick"):
            assert v[k].tobytes() == p[k].tobytes(), (tag, k)
        if not v["keys"]:
            continue
        rows = _winner_rows_of(v)
        ref, votes, A = V.box_vote(v["bb"], rows + 1, VOTE["overlap"], 5, V.LOG_SCORE, v["kc"], v["r2"])
        assert np.array_equal(v["votes"][rows], votes), tag
        for q, key in enumerate(v["keys"]):
            got = np.array(key[4:8])
            if votes[q] < 2:
                assert got.tobytes() == v["r2"][rows[q]].tobytes(), "%s winner %d: fewer than two voters" % (tag, q)
                continue
            moved += got.tobytes() != v["r2"][rows[q]].tobytes()
            for c in range(4):
                bound = V.rect_error_bound(int(votes[q]), A[q, c], V.LOG_SCORE)
                assert abs(got[c] - ref[q, c]) <= bound, "%s winner %d coordinate %d" % (tag, q, c)
            voters = np.nonzero(V.membership_f32(v["bb"], int(rows[q]), VOTE["overlap"], v["kc"]))[0]
            crossed += len(set(T.view_of(int(v["keep_row"][j]) + 1, v["roff"]) for j in voters)) > 1
    print("voting under %r: %d winners whose voters come from more than one view, %d moved" % (BOTH, crossed, moved))
    assert crossed > 0 and moved > 0, "no winner has voters of two views: nothing is exercised"


def test_gaussian_soft_nms_in_score_order_with_voting_across_views(F, setup):
    s = setup
    kw = dict(tta=BOTH, nms=dict(method="gaussian"), proposals=dict(order="score"))
    soft = _tta_collect(F, F.Detector(s["model"], **kw), s["frames"])
    voted = _tta_collect(F, F.Detector(s["model"], box_voting=VOTE, **kw), s["frames"])
    method, overlap, sigma, min_score, _ = F.Detector.nms_settings(kw["nms"])
    winners = crossed = 0
    for b, (v, p) in enumerate(zip(voted, soft)):
        tag = "frame %d" % b
        assert [k[:4] for k in v["keys"]] == [k[:4] for k in p["keys"]], tag
        if p["kept"] == 0:
            continue
        # gaussian decay of log-scores is exact in fp32 (soft_nms_ref.is_exact): picks and decayed confidences bit for bit
        assert S.is_exact(S.METHODS.index("gaussian"), 1)
        pick, sc = S.soft_nms_f32(p["bb"], 5, S.METHODS.index("gaussian"), overlap, sigma, float(np.log(min_score)), 1, p["kc"])
        order = np.argsort(p["kc"][pick - 1], kind="stable")           # classes ascending, pick order within a class
        want = [(int(p["kc"][j]), float(np.float32(c)), int(p["keep_row"][j]) + 1) for j, c in zip((pick - 1)[order], sc[order])]
        assert [k[:3] for k in p["keys"]] == want, tag
        assert [k[4:8] for k in p["keys"]] == [tuple(p["r2"][j].tolist()) for j in (pick - 1)[order]], tag
        winners += len(want)
        rows = (pick - 1)[order]
        ref, votes, A = V.box_vote(v["bb"], rows + 1, VOTE["overlap"], 5, V.LOG_SCORE, v["kc"], v["r2"])
        assert np.array_equal(v["votes"][rows], votes), tag
        for q, key in enumerate(v["keys"]):
            for c in range(4):
                assert abs(key[4 + c] - ref[q, c]) <= V.rect_error_bound(int(votes[q]), A[q, c], V.LOG_SCORE), (tag, q, c)
            if votes[q] > 1:
                voters = np.nonzero(V.membership_f32(v["bb"], int(rows[q]), VOTE["overlap"], v["kc"]))[0]
                crossed += len(set(T.view_of(int(v["keep_row"][j]) + 1, v["roff"]) for j in voters)) > 1
    print("gaussian + score order + voting: %d winners, %d with voters of more than one view" % (winners, crossed))
    assert winners > 0 and crossed > 0


def test_settings_combine_with_the_key(F, setup):
    """shared_cnet, the caps, all-class scoring and max_detections run with the key as they run without: detect_batch equals
    the detect loop under each (shared_cnet: it runs)"""
    s = setup
    frames = s["frames"][:3]
    for kw in (dict(proposals=dict(order="score", pre_nms_top_n=40, post_nms_top_n=20)),
               dict(scoring=dict(classes="all", min_confidence=0.05, max_detections=5))):
        want = _tta_collect(F, F.Detector(s["model"], tta=FLIP, **kw), frames)
        d = F.Detector(s["model"], tta=FLIP, **kw)
        res = d.detect_batch(frames)
        for b in range(len(frames)):
            _same_state(_frame_state(res[b], d.last_batch[b]), want[b], "%r frame %d" % (kw, b))
        assert sum(len(w["keys"]) for w in want) > 0
    res = F.Detector(s["model"], tta=FLIP).detect_batch(frames, shared_cnet=True)
    assert sum(len(x) for x in res) > 0 and all("view" in x for r in res for x in r)


def test_evaluate_detections_in_batches(F, setup):
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import evaluate_detections
    s = setup
    d = F.Detector(s["model"], tta=FLIP)
    items = []
    for img in s["frames"]:
        rois = []
        for j, x in enumerate(list(d.detect(img))[::3]):
            r = x["r2"]
            rois.append(F.Roi(Rect(r.minX, r.minY, r.maxX, r.maxY) if j % 2 == 0 else r.offset(r.width() * 0.3, 0), x["class"]))
        rois.append(F.Roi(Rect(5, 5, 40, 40), 16))
        items.append(dict(img=img, rois=rois))
    one = evaluate_detections(F.Detector(s["model"], tta=FLIP), _Val(items), len(items), batch=1)
    assert one["detections"] > 0 and one["mAP"] > 0
    four = evaluate_detections(F.Detector(s["model"], tta=FLIP), _Val(items), len(items), batch=4)
    assert four == one
