"""The class test of a chunk in one launch (frcnn_detect_classes_batch, cfg.scoring).  Op level, on the problems of
tests/detect_classes_ref.py (their input conditions are asserted in test_detect_classes_host.py): decisions, order, kc, keep_row
and the confidence column against the restatement, exact; r2 and the fp32 boxes against frcnn_detect_post on the same candidates,
bit for bit; mode 0 against the pair frcnn_cnet_decode + frcnn_detect_post, whole output.  Counts on both sides of a wave (64)
and of a tile (1024).  Detector level (the fixture pattern of test_gpu_soft_nms.py, with four classes so that the net's mass is
shared): the key absent and the empty table change nothing, "all" at one half is "top" at one half, "all" at 0.05 is the
restatement's rows run through nms() per class, detect_batch is the detect() loop under every other setting."""
import ctypes as C
import math

import numpy as np
import pytest

import detect_classes_ref as D
from test_gpu_detect_batch import _amplified_weights, _frames, _winner_rows
from test_gpu_proposals import _collect, _launches, _same
from test_gpu_soft_nms import H, SEEDS, W, _winner_keys

pytestmark = pytest.mark.gpu
SENT = -7
TILE = 1024           # DC_THREADS of csrc/detect.hip: candidates per tile
GROUP = 32            # DC_GROUP: frames per launch


# ------------------------------------------------------------------------------------------------ op level
def _run(F, frames, ncls, min_conf, mode, row_stride, packed=False, bg=None, total=True):
    """frcnn_detect_classes_batch on the frames (problems of detect_classes_ref.problem, or None: no candidates) -> one dict per
    frame (bb, kc, keep_row, r2: the frame's row_stride rows; K, total).  The net's outputs lie at b * (Rmax + 3) rows, or
    (packed) at the prefix sum of the counts; the rows between hold log-probabilities of 0 (they would pass any threshold) and
    every output is filled with a sentinel; asserts that the guard tails and the inputs are untouched."""
    B = len(frames)
    Rs = [0 if P is None else len(P["lp"]) for P in frames]
    gap = max(Rs) + 3
    row0 = [int(np.sum(Rs[:b])) if packed else b * gap for b in range(B)]
    nrows = (sum(Rs) if packed else B * gap) + 1
    lp, bbox = np.zeros((nrows, ncls), np.float32), np.full((nrows, 4), 0.25, np.float32)
    ms = max([len(P["rect"]) for P in frames if P is not None] + [1]) + 5
    rect, pick = np.full((B * ms, 4), 3.0, np.float64), np.ones(B * ms, np.int64)
    for b, P in enumerate(frames):
        if P is not None:
            lp[row0[b]:row0[b] + Rs[b]], bbox[row0[b]:row0[b] + Rs[b]] = P["lp"], P["bbox"]
            rect[b * ms:b * ms + len(P["rect"])], pick[b * ms:b * ms + Rs[b]] = P["rect"], P["pick"]
    n = B * row_stride + 8
    host = dict(bb=np.full((n, 5), SENT, np.float32), kc=np.full(n, SENT, np.int32), keep_row=np.full(n, SENT, np.int32),
                r2=np.full((n, 4), SENT, np.float64), K=np.full(B + 2, SENT, np.int32), total=np.full(B + 2, SENT, np.int32))
    dev = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in host.items())
    ins = [F.DeviceTensor.from_numpy(a) for a in (lp, bbox, rect, pick)]
    F._lib.call("frcnn_detect_classes_batch", F.ptr(ins[0]), F.ptr(ins[1]), (C.c_int * B)(*Rs), (C.c_longlong * B)(*row0), B,
                F.ptr(ins[2]), F.ptr(ins[3]), ms, ncls, ncls if bg is None else bg, float(min_conf), mode, F.ptr(dev["bb"]),
                F.ptr(dev["kc"]), F.ptr(dev["keep_row"]), F.ptr(dev["r2"]), row_stride, F.ptr(dev["K"]),
                F.ptr(dev["total"]) if total else None, F.stream_ptr())
    got = dict((k, t.numpy()) for k, t in dev.items())
    for t, a in zip(ins, (lp, bbox, rect, pick)):
        assert t.numpy().tobytes() == a.tobytes(), "an input was written"
    for k in ("bb", "kc", "keep_row", "r2"):
        assert np.all(got[k][B * row_stride:] == SENT), "%s: stores behind the last frame" % k
    assert np.all(got["K"][B:] == SENT) and np.all(got["total"][B:] == SENT)
    if not total:
        assert np.all(got["total"] == SENT)
    out = []
    for b in range(B):
        seg = slice(b * row_stride, (b + 1) * row_stride)
        out.append(dict(bb=got["bb"][seg], kc=got["kc"][seg], keep_row=got["keep_row"][seg], r2=got["r2"][seg], K=int(got["K"][b]),
                        total=int(got["total"][b])))
    return out


_decoded = {}


def _decode_all(F, P):
    """(r2 R x 4 fp64, boxes R x 4 fp32) of EVERY candidate of a problem from frcnn_detect_post (class 1 at confidence 0 for all:
    each survives, in order) -- worked out once per problem"""
    key = id(P)
    if key not in _decoded:
        R = len(P["lp"])
        d = [F.DeviceTensor.from_numpy(a) for a in (np.ones(R, np.int32), np.zeros(R, np.float32), P["bbox"], P["rect"], P["pick"])]
        bb, kc, kr = F.DeviceTensor.empty((R, 5), np.float32), F.DeviceTensor.empty((R,), np.int32), F.DeviceTensor.empty((R,), np.int32)
        r2, K = F.DeviceTensor.empty((R, 4), np.float64), F.DeviceTensor.empty((1,), np.int32)
        F._lib.call("frcnn_detect_post", *([F.ptr(t) for t in d] + [R, 2, 0.5] + [F.ptr(t) for t in (bb, kc, kr, r2, K)] + [F.stream_ptr()]))
        assert int(K.numpy()[0]) == R and kr.numpy().tolist() == list(range(R))
        _decoded[key] = (P, r2.numpy(), bb.numpy()[:, :4].copy())
    return _decoded[key][1:]


def _check(F, got, P, ncls, min_conf, mode, row_stride, tag, bg=None):
    """one frame of _run against the restatement and frcnn_detect_post; -> the restatement's dict"""
    if P is None:
        assert got["K"] == 0 and got["total"] in (0, SENT), tag
        for k in ("bb", "kc", "keep_row", "r2"):
            assert np.all(got[k] == SENT), "%s: %s of a frame without candidates" % (tag, k)
        return None
    ref = D.detect_classes(P["lp"], ncls if bg is None else bg, min_conf, mode, row_stride)
    K = ref["K"]
    assert got["K"] == K and got["total"] in (ref["total"], SENT), "%s: K %d total %d, expected %d %d" % (
        tag, got["K"], got["total"], K, ref["total"])
    assert np.array_equal(got["keep_row"][:K], ref["cand"]) and np.array_equal(got["kc"][:K], ref["cls"]), "%s: rows" % tag
    assert got["bb"][:K, 4].tobytes() == ref["conf"].tobytes(), "%s: confidences" % tag
    r2, boxes = _decode_all(F, P)
    assert got["r2"][:K].tobytes() == r2[ref["cand"]].tobytes(), "%s: r2" % tag
    assert got["bb"][:K, :4].tobytes() == boxes[ref["cand"]].tobytes(), "%s: boxes" % tag
    for k in ("bb", "kc", "keep_row", "r2"):
        assert np.all(got[k][K:] == SENT), "%s: %s behind row K" % (tag, k)
    return ref


_problems = {}


def _problem(R, ncls, nan_row=True):
    key = (R, ncls, nan_row)
    if key not in _problems:
        _problems[key] = D.problem(D.case_seed(R, ncls), R, ncls, nan_row=nan_row)
    return _problems[key]


@pytest.mark.parametrize("R", D.SIZES)
def test_sizes_classes_and_thresholds_against_the_restatement(F, R):
    multi = rows = 0
    for ncls in D.NCLS:
        P = _problem(R, ncls)
        for c in D.MIN_CONF:
            for mode in (D.TOP, D.ALL):
                stride = R * D.max_rows(ncls, c) if mode == D.ALL else R
                tag = "R %d ncls %d min_conf %g mode %d" % (R, ncls, c, mode)
                ref = _check(F, _run(F, [P], ncls, c, mode, stride)[0], P, ncls, c, mode, stride, tag)
                assert ref["total"] <= stride, "%s: the stride Detector sizes its buffers by overflows" % tag
                rows += ref["total"]
                multi += int(mode == D.ALL and ref["per_candidate"].max() >= 2)
    print("R = %d: %d rows, %d problems with several rows a candidate" % (R, rows, multi))
    assert rows > 0 and (R < 63 or multi > 0)


@pytest.mark.parametrize("R", [1, 65, 1025, 2300])
def test_mode_0_is_decode_plus_post(F, R):
    """the whole output of mode 0 is that of frcnn_cnet_decode + frcnn_detect_post, bit for bit (a NaN row included)"""
    for ncls in D.NCLS:
        P = _problem(R, ncls)
        d = [F.DeviceTensor.from_numpy(P[k]) for k in ("lp", "bbox", "rect", "pick")]
        for c in (0.0, 0.2):
            cls, conf = F.DeviceTensor.empty((R,), np.int32), F.DeviceTensor.empty((R,), np.float32)
            want = dict(bb=np.full((R, 5), SENT, np.float32), kc=np.full(R, SENT, np.int32), keep_row=np.full(R, SENT, np.int32),
                        r2=np.full((R, 4), SENT, np.float64), K=np.full(1, SENT, np.int32))
            w = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in want.items())
            F._lib.call("frcnn_cnet_decode", F.ptr(d[0]), R, ncls, F.ptr(cls), F.ptr(conf), F.stream_ptr())
            F._lib.call("frcnn_detect_post", F.ptr(cls), F.ptr(conf), F.ptr(d[1]), F.ptr(d[2]), F.ptr(d[3]), R, ncls, c, F.ptr(w["bb"]),
                        F.ptr(w["kc"]), F.ptr(w["keep_row"]), F.ptr(w["r2"]), F.ptr(w["K"]), F.stream_ptr())
            got = _run(F, [P], ncls, c, D.TOP, R)[0]
            for k in ("bb", "kc", "keep_row", "r2"):
                assert got[k].tobytes() == w[k].numpy().tobytes(), "R %d ncls %d min_conf %g: %s" % (R, ncls, c, k)
            assert got["K"] == int(w["K"].numpy()[0]) == got["total"]


def test_three_frames_with_an_empty_one_packed_and_strided(F):
    """B = 3, the middle frame without candidates, strides larger than the counts; the packed layout (row0 = the prefix sum of the
    counts, as under shared_cnet) gives the rows of the strided one"""
    for ncls in D.NCLS:
        frames = [_problem(65, ncls), None, _problem(1025, ncls)]
        for mode, c in ((D.ALL, 0.05), (D.TOP, 0.2), (D.ALL, 0.0)):
            stride = 1025 * (ncls - 1) + 11
            runs = [_run(F, frames, ncls, c, mode, stride, packed=p) for p in (False, True)]
            for b in range(3):
                _check(F, runs[0][b], frames[b], ncls, c, mode, stride, "strided ncls %d mode %d frame %d" % (ncls, mode, b))
                for k in ("bb", "kc", "keep_row", "r2"):
                    assert runs[1][b][k].tobytes() == runs[0][b][k].tobytes(), (ncls, mode, b, k)
                assert runs[1][b]["K"] == runs[0][b]["K"] and runs[1][b]["total"] == runs[0][b]["total"]
    # no frame has candidates: the counts are written, nothing else; total_dev may be NULL
    for got in _run(F, [None, None], 5, 0.2, D.ALL, 4) + _run(F, [None], 5, 0.2, D.TOP, 0, total=False):
        _check(F, got, None, 5, 0.2, D.ALL, 4, "no candidates")


@pytest.mark.parametrize("R", [65, 1025])
def test_a_row_stride_smaller_than_the_total(F, R):
    for ncls, c in ((5, 0.05), (17, 0.0)):
        P = _problem(R, ncls)
        full = D.detect_classes(P["lp"], ncls, c, D.ALL)
        assert full["total"] > R
        for stride in (0, 1, R, full["total"] - 1, full["total"]):
            got = _run(F, [P], ncls, c, D.ALL, stride)[0]
            ref = _check(F, got, P, ncls, c, D.ALL, stride, "R %d ncls %d stride %d" % (R, ncls, stride))
            assert got["K"] == min(stride, full["total"]) and got["total"] == full["total"] == ref["total"]
        top = D.detect_classes(P["lp"], ncls, c, D.TOP)
        got = _run(F, [P], ncls, c, D.TOP, top["total"] // 2)[0]
        _check(F, got, P, ncls, c, D.TOP, top["total"] // 2, "top, half the rows")
        assert got["K"] == top["total"] // 2 and got["total"] == top["total"]


def test_a_frame_does_not_depend_on_its_slot_or_its_neighbours(F):
    """the same frame alone, last of three, and behind a launch group's boundary (frame 33 of 34): bit-identical rows"""
    ncls, c = 5, 0.05
    P = _problem(1025, ncls)
    stride = 1025 * (ncls - 1)
    alone = _run(F, [P], ncls, c, D.ALL, stride)[0]
    _check(F, alone, P, ncls, c, D.ALL, stride, "alone")
    small = [D.problem(900 + b, 3 + 5 * b, ncls, special=False) for b in range(GROUP + 1)]
    for frames in ([_problem(2300, ncls), _problem(63, ncls), P], small + [P]):
        got = _run(F, frames, ncls, c, D.ALL, stride, packed=len(frames) > 3)
        for k in ("bb", "kc", "keep_row", "r2"):
            assert got[-1][k].tobytes() == alone[k].tobytes(), (len(frames), k)
        assert got[-1]["K"] == alone["K"] and got[-1]["total"] == alone["total"]
        for b, Q in enumerate(frames[:-1]):
            _check(F, got[b], Q, ncls, c, D.ALL, stride, "B %d frame %d" % (len(frames), b))


def test_another_background_class(F):
    P = _problem(65, 5, nan_row=False)
    for bg in (1, 3):
        for mode in (D.TOP, D.ALL):
            ref = _check(F, _run(F, [P], 5, 0.05, mode, 65 * 4, bg=bg)[0], P, 5, 0.05, mode, 65 * 4, "bg %d mode %d" % (bg, mode), bg=bg)
            assert ref["total"] > 0 and np.all(ref["cls"] != bg)


def test_argument_errors_launch_nothing_and_store_nothing(F):
    R = 16
    P = D.problem(1, R, 5)
    ins = dict((k, F.DeviceTensor.from_numpy(P[k])) for k in ("lp", "bbox", "rect", "pick"))
    outs = dict(bb=np.full((64, 5), SENT, np.float32), kc=np.full(64, SENT, np.int32), keep_row=np.full(64, SENT, np.int32),
                r2=np.full((64, 4), SENT, np.float64), K=np.full(4, SENT, np.int32), total=np.full(4, SENT, np.int32))
    dev = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in outs.items())
    arr = lambda t, v: (t * len(v))(*v)
    good = dict(cls_out=F.ptr(ins["lp"]), bbox=F.ptr(ins["bbox"]), R=arr(C.c_int, [R]), row0=arr(C.c_longlong, [0]), B=1,
                rect=F.ptr(ins["rect"]), pick=F.ptr(ins["pick"]), match_stride=len(P["rect"]), ncls=5, bgclass=5, min_conf=0.2, mode=1,
                bb=F.ptr(dev["bb"]), kc=F.ptr(dev["kc"]), keep_row=F.ptr(dev["keep_row"]), r2=F.ptr(dev["r2"]), row_stride=64,
                K_dev=F.ptr(dev["K"]), total_dev=F.ptr(dev["total"]))
    bad = [dict(B=-1), dict(B=65536), dict(ncls=1), dict(ncls=0), dict(bgclass=0), dict(bgclass=6), dict(bgclass=-1), dict(mode=2),
           dict(mode=-1), dict(row_stride=-1), dict(match_stride=-1), dict(R=arr(C.c_int, [-1])), dict(row0=arr(C.c_longlong, [-1])),
           dict(R=None), dict(row0=None), dict(K_dev=None), dict(cls_out=None), dict(bbox=None), dict(rect=None), dict(pick=None),
           dict(bb=None), dict(kc=None), dict(keep_row=None), dict(r2=None),
           dict(B=2, R=arr(C.c_int, [R, -2]), row0=arr(C.c_longlong, [0, 0]))]     # (a bad second frame: the first is not run either)

    def call(args):
        F._lib.call("frcnn_detect_classes_batch", *(list(args.values()) + [F.stream_ptr()]))

    def errors():
        for t in bad:
            with pytest.raises(F.FrcnnError):
                call(dict(good, **t))
    la = _launches(F, errors)
    assert sum(la.values()) == 0, la
    for k, t in dev.items():
        assert np.all(t.numpy() == SENT), "an argument error stored something (%s)" % k
    # the counter does count, under the class of detect_post; B = 0 is no error and no launch; total_dev may be NULL; more than GROUP
    # frames take a launch per group
    counts = F.DeviceTensor.empty((GROUP + 1,), np.int32)
    many = dict(good, B=GROUP + 1, R=arr(C.c_int, [0] * (GROUP + 1)), row0=arr(C.c_longlong, [0] * (GROUP + 1)), K_dev=F.ptr(counts),
                total_dev=None)
    la = _launches(F, lambda: (call(good), call(dict(good, B=0)), call(dict(good, total_dev=None)), call(many)))
    assert la["elemwise"] == 4 and sum(la.values()) == 4, la
    ref = D.detect_classes(P["lp"], 5, 0.2, D.ALL)
    assert dev["K"].numpy().tolist() == [ref["K"], SENT, SENT, SENT] and dev["total"].numpy()[0] == ref["total"]
    assert not counts.numpy().any()


# ------------------------------------------------------------------------------------------------ Detector level
CLASSES = 4       # four classes and the background: an untrained net shares its mass among them
# Gain of the class head (_amplified_weights).  The foreground classes of the untrained net lie within a few percent of each other
# and the gain moves the background against them: at 12 the background is the arg-max of about a third of the candidates, and
# every candidate holds several classes over 0.05.  A large negative gain removes the background and spreads the foreground
# classes: at HALF_GAIN some candidates have a class over one half.
GAIN = 12.0
HALF_GAIN = -1000.0
ALL05 = dict(classes="all", min_confidence=0.05)


@pytest.fixture(scope="module")
def setup(F):
    import torch
    cfg = dict(F.duplo_cfg, class_count=CLASSES)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    weights.copy_(torch.from_numpy(_amplified_weights(model["native"], w, CLASSES + 1, cls_gain=GAIN)))
    frames = _frames(F, SEEDS, H, W)
    s = dict(cfg=cfg, model=model, weights=weights, gradient=gradient, frames=frames, w=w)
    s["plain"] = _collect(F.Detector(model), frames)
    s["all"] = _collect(F.Detector(model, scoring=ALL05), frames)
    print("scoring: candidates %s, survivors %s -> %s under \"all\" at 0.05, winners %s -> %s"
          % ([len(r["pick"]) for r in s["plain"]], [r["kept"] for r in s["plain"]], [r["kept"] for r in s["all"]],
             [r["nwin"] for r in s["plain"]], [r["nwin"] for r in s["all"]]))
    return s


def _several_rows(records, min_conf=0.05):
    """the candidates of the frames (dicts of _collect) that emit at least two rows under "all" """
    return sum(int(np.sum(D.detect_classes(r["cnet"]["cls"], CLASSES + 1, min_conf, D.ALL)["per_candidate"] >= 2))
               for r in records if r["cnet"] is not None)


def test_key_absent_and_empty_table_change_nothing(F, setup):
    s = setup
    got = {}

    def run(name, d):
        def fn():
            got[name] = _collect(d, s["frames"])
            got[name + "/batch"] = d.detect_batch(s["frames"])
        return _launches(F, fn)
    plain = F.Detector(s["model"])
    la0 = run("plain", plain)
    assert plain.scoring is None
    la1 = run("none", F.Detector(s["model"], scoring=None))
    la2 = run("cfg none", F.Detector(dict(s["model"], cfg=dict(s["cfg"], scoring=None))))
    assert la0 == la1 == la2, "the same launches per kernel class"
    empty = F.Detector(s["model"], scoring={})
    assert empty.scoring == ("top", 0.2, None)
    la3 = run("empty", empty)
    for name in ("plain", "none", "cfg none", "empty"):
        _same(got[name], s["plain"], name)
        for b in range(len(SEEDS)):
            assert _winner_rows(got[name + "/batch"][b]) == s["plain"][b]["winners"], (name, b)
    # the launches saved: decode + post per frame with matches become one per chunk (the loop: 8 chunks of one frame; the batch: one)
    # (a frame without matches costs the per-frame path one frcnn_zero of its count in a chunk that has candidates)
    busy = sum(r["n"] > 0 for r in s["plain"])
    idle = len(SEEDS) - busy
    assert busy > 1 and sum(r["nwin"] for r in s["plain"]) > 0
    assert la0["elemwise"] - la3["elemwise"] == (2 * busy - busy) + (2 * busy + idle - 1), (la0, la3)
    assert dict(la0, elemwise=0) == dict(la3, elemwise=0)
    # the cfg's key is read when the call names none, and the call's table wins
    m = dict(s["model"], cfg=dict(s["cfg"], scoring=dict(classes="all")))
    assert F.Detector(m).scoring == ("all", 0.2, None) and F.Detector(m, scoring=dict(min_confidence=0.1)).scoring == ("top", 0.1, None)


def test_all_at_one_half_is_top_at_one_half(F, setup):
    """at most one class exceeds one half, and it is the arg-max"""
    import torch
    s = setup
    nat, live = s["model"]["native"], s["weights"]
    try:      # (the module's weights with another gain of the class head, put back below)
        live.copy_(torch.from_numpy(_amplified_weights(nat, s["w"], CLASSES + 1, cls_gain=HALF_GAIN)))
        top = _collect(F.Detector(s["model"], scoring=dict(min_confidence=0.5)), s["frames"])
        every = _collect(F.Detector(s["model"], scoring=dict(classes="all", min_confidence=0.5)), s["frames"])
        low = _collect(F.Detector(s["model"], scoring=ALL05), s["frames"])
    finally:
        live.copy_(torch.from_numpy(_amplified_weights(nat, s["w"], CLASSES + 1, cls_gain=GAIN)))
    _same(every, top, "all at 0.5")
    assert _several_rows(low) > 0, "no candidate yields two rows at 0.05"
    assert sum(r["nwin"] for r in top) > 0, "no winner at one half: nothing is compared"
    assert sum(r["kept"] for r in low) > sum(r["kept"] for r in top)


def _host_winners(F, r, scoring, overlap=0.1):
    """What the host derives from a frame's OWN classification-net outputs (r: a dict of _collect, or a record): the restatement's
    rows, Anchors.anchorToInput in double, nms() per class on the fp32 boxes -> ([(class, candidate 1-based)], r2 of each, their
    confidences, the restatement's dict)"""
    bbox, logp = r["cnet"]["bbox"], r["cnet"]["cls"]
    ref = D.detect_classes(logp, CLASSES + 1, scoring["min_confidence"], D.ALL if scoring["classes"] == "all" else D.TOP)
    keep = ref["cand"]
    ra = r["rect"][r["pick"][keep] - 1]
    aw, ah = ra[:, 2] - ra[:, 0], ra[:, 3] - ra[:, 1]
    t = bbox[keep].astype(np.float64)
    x0 = t[:, 0] * aw + ra[:, 0]; y0 = t[:, 1] * ah + ra[:, 1]
    ew = np.array([math.exp(v) for v in t[:, 2].tolist()]) * aw; eh = np.array([math.exp(v) for v in t[:, 3].tolist()]) * ah
    r2 = np.stack([x0, y0, x0 + ew, y0 + eh], 1).reshape(-1, 4)
    bb = r2.astype(np.float32)
    want, rows_of = [], []
    for c in sorted(set(ref["cls"].tolist())):
        rows = np.nonzero(ref["cls"] == c)[0]
        for i in F.nms(bb[rows], overlap).tolist():
            want.append((c, int(keep[rows[i - 1]]) + 1))
            rows_of.append(int(rows[i - 1]))
    return want, r2[rows_of], [float(ref["conf"][j]) for j in rows_of], ref


def _assert_host_winners(F, r, winners, scoring, tag):
    """winners: tuples of _winner_rows"""
    keys = _winner_keys(winners)
    want, r2, conf, ref = _host_winners(F, r, scoring)
    assert r["kept"] == ref["total"], tag
    assert [(k[0], k[1]) for k in keys] == want, tag
    assert [k[2] for k in keys] == conf, tag
    if want:
        assert np.allclose(np.array([k[3] for k in keys]), r2, rtol=2e-15, atol=0), "%s: r2" % tag
    return ref


def test_all_at_005_is_the_restatement_through_nms_per_class(F, setup):
    s = setup
    top = _collect(F.Detector(s["model"], scoring=dict(min_confidence=0.05)), s["frames"])
    several = shared = background = 0
    for b, (r, t) in enumerate(zip(s["all"], top)):
        tag = "frame %d" % b
        if r["cnet"] is None:
            assert r["nwin"] == 0
            continue
        assert np.array_equal(r["cnet"]["cls"], t["cnet"]["cls"]), tag       # (everything in front of the class test is the same)
        ref = _assert_host_winners(F, r, r["winners"], ALL05, tag)
        rt = _assert_host_winners(F, t, t["winners"], dict(classes="top", min_confidence=0.05), tag + " top")
        # a superset of "top"'s class-test survivors
        assert set(zip(rt["cand"].tolist(), rt["cls"].tolist())) <= set(zip(ref["cand"].tolist(), ref["cls"].tolist())), tag
        assert r["kept"] >= t["kept"]
        assert ref["per_candidate"].max() <= D.max_rows(CLASSES + 1, 0.05), tag
        several += int(np.sum(ref["per_candidate"] >= 2))
        background += int(np.sum((D.first_max(r["cnet"]["cls"]) == CLASSES) & (ref["per_candidate"] > 0)))
        # winners that share a candidate carry its one r2, bit for bit, under different classes
        by = {}
        for k in _winner_keys(r["winners"]):
            by.setdefault(k[1], []).append(k)
        for ks in by.values():
            assert len(set(k[3] for k in ks)) == 1 and len(set(k[0] for k in ks)) == len(ks), tag
            shared += len(ks) > 1
    print("\"all\" at 0.05: %d candidates with several rows, %d with a background arg-max and a row, %d shared by winners"
          % (several, background, shared))
    assert several > 0, "no candidate yields two rows"
    assert shared > 0, "no two winners share a candidate"


COMBOS = {"all": dict(scoring=ALL05),
          "all+gaussian": dict(scoring=ALL05, nms=dict(method="gaussian")),
          "all+voting": dict(scoring=ALL05, box_voting=dict(overlap=0.1)),
          "all+score": dict(scoring=dict(ALL05, max_detections=5), proposals=dict(order="score", pre_nms_top_n=50, post_nms_top_n=20))}


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_detect_batch_equals_the_detect_loop(F, setup, combo):
    s = setup
    kw = COMBOS[combo]
    want = _collect(F.Detector(s["model"], **kw), s["frames"])
    assert sum(r["nwin"] for r in want) > 0 and _several_rows(want) > 0, "no candidate yields two rows"
    for batch in (8, 3):
        d = F.Detector(s["model"], **kw)
        d.BATCH = batch
        res = d.detect_batch(s["frames"])
        for b, (rec, win, w) in enumerate(zip(d.last_batch, res, want)):
            tag = "%s BATCH %d frame %d" % (combo, batch, b)
            assert _winner_rows(win) == w["winners"], tag
            assert rec["n"] == w["n"] and rec["kept"] == w["kept"] and np.array_equal(rec["pick"], w["pick"]), tag


def test_detect_batch_of_mixed_sizes_equals_the_detect_loop(F, setup):
    s = setup
    frames = [F.synthetic_image(h, w, k) for k, (h, w) in zip(SEEDS, [(H, W), (128, 192), (144, 176), (176, 128)] * 2)]
    want = _collect(F.Detector(s["model"], scoring=ALL05), frames)
    assert sum(r["nwin"] for r in want) > 0 and _several_rows(want) > 0, "no candidate yields two rows"
    d = F.Detector(s["model"], scoring=ALL05)
    res = d.detect_batch(frames, mixed_sizes=True)
    for b, (rec, win, w) in enumerate(zip(d.last_batch, res, want)):
        assert _winner_rows(win) == w["winners"] and rec["kept"] == w["kept"], b


def test_shared_cnet_winners_follow_from_its_own_outputs(F, setup):
    """the shared pass's outputs differ from detect()'s within the net's error: every frame is judged against its own record"""
    s = setup
    d = F.Detector(s["model"], scoring=ALL05)
    res = d.detect_batch(s["frames"], shared_cnet=True)
    several = 0
    for b, (rec, win) in enumerate(zip(d.last_batch, res)):
        if rec["n"] == 0:
            assert win == []
            continue
        ref = _assert_host_winners(F, rec, _winner_rows(win), ALL05, "shared frame %d" % b)
        several += int(np.sum(ref["per_candidate"] >= 2))
    assert several > 0 and sum(len(w) for w in res) > 0, "no candidate yields two rows"


def test_max_detections_keeps_the_best(F, setup):
    s = setup
    assert _several_rows(s["all"]) > 0, "no candidate yields two rows"
    cut = 0
    for M in (1, 3, 1000):
        got = _collect(F.Detector(s["model"], scoring=dict(ALL05, max_detections=M)), s["frames"])
        for b, (g, w) in enumerate(zip(got, s["all"])):
            conf = np.array([x[1] for x in w["winners"]], np.float32)
            assert g["kept"] == w["kept"]
            if len(conf) <= M:
                assert g["winners"] == w["winners"], (M, b)
                continue
            cut += 1
            order = np.argsort(-conf, kind="stable")
            assert conf[order[M - 1]] > conf[order[M]], "a tie at the cut: the fixture does not decide it"   # (ties: the host test)
            assert g["winners"] == [w["winners"][j] for j in sorted(order[:M].tolist())], (M, b)    # still classes ascending
    assert cut > 0


def test_refusals_come_before_the_per_class_pass(F, setup):
    s = setup
    frame = next(f for f, r in zip(s["frames"], s["plain"]) if r["nwin"] > 0)
    first = _launches(F, lambda: F.Detector(s["model"]).proposals(frame))
    d = F.Detector(s["model"], scoring=ALL05)
    d.CLASS_NMS_WORKSPACE = 64
    d2 = F.Detector(s["model"], scoring=ALL05, nms=dict(method="linear"))
    d2.SOFT_NMS_ROWS = 1
    for det in (d, d2):
        def refused():
            with pytest.raises(F.FrcnnError, match="post_nms_top_n"):
                det.detect(frame)
        la = _launches(F, refused)
        assert la["nms"] == first["nms"] and la["soft_nms"] == 0, la
    # the limits as they stand refuse nothing here, and without the key the workspace is not looked at
    plain = F.Detector(s["model"])
    plain.CLASS_NMS_WORKSPACE = 64
    assert len(plain.detect(frame)) > 0 and len(F.Detector(s["model"], scoring=ALL05).detect(frame)) > 0
