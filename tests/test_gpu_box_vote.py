"""Box voting on the device (frcnn_box_vote_batch, cfg.box_voting).  Kernel level, against the restatement of
tests/box_vote_ref.py: who votes (and so `votes`) bit for bit, every coordinate within the bound derived there, a winner with
fewer than two voters its own rect bit for bit, nothing stored outside the winners' rows.  Counts on both sides of the lane
boundary (64 rows) and of the LDS tier's cap (2048 | 2049).  Detector level (the fixture pattern of test_gpu_soft_nms.py:
vgg_small, amplified weights, 128x176 frames): the key absent changes nothing and launches nothing new; with the key every
winner keeps everything but r2, and r2 is the restatement's on the record's own arrays."""
import ctypes as C

import numpy as np
import pytest

import box_vote_ref as V
from soft_nms_ref import clustered_boxes, disjoint_boxes, grid_scores, rows5
from test_gpu_detect_batch import _Val, _amplified_weights, _frames, _winner_rows
from test_gpu_proposals import _collect, _launches, _same
from test_gpu_soft_nms import H, SEEDS, W, _classes, _winner_keys

pytestmark = pytest.mark.gpu
SENT = -7
LANES = 64            # BV_LANES of csrc/box_vote.hip: lane l takes rows l, l + 64, ...
WAVES = 4             # BV_WAVES: winners per block
LDS_ROWS = 2048       # BV_LDS_ROWS: the largest segment staged in LDS
SIZES = (1, 2, 63, 64, 65, 129, 2048, 2049)      # (LANES - 1, LANES, LANES + 1, 2 * LANES + 1, LDS_ROWS, LDS_ROWS + 1)
MANY = 0.2            # an overlap at which the clusters of clustered_boxes hold several voters each


def _inputs(kind, seed, n, mode):
    """rows n x 5: boxes of soft_nms_ref's generators, distinct scores -- probabilities, or their range as logs under mode 2"""
    rng = np.random.RandomState(seed)
    boxes = clustered_boxes(rng, n) if kind == "clustered" else disjoint_boxes(rng, n)
    sc = grid_scores(rng, n, -1.6, -0.01) if mode == V.LOG_SCORE else grid_scores(rng, n, 0.05, 1.0)
    return rows5(boxes, sc)


def _rects(rng, rows):
    """fp64 coordinates that differ from the fp32 boxes in the low bits"""
    return rows[:, :4].astype(np.float64) + rng.uniform(-1.0, 1.0, (len(rows), 4)) * 2.0 ** -20


def _run(F, rows, B, stride, n_cap, counts, picks, mode, overlap, cls=None, rect=None, score_col=5, votes=True):
    """frcnn_box_vote_batch on host arrays (rows: [B * stride][ncols]; picks: one int64 array of 1-based rows per segment, wins =
    their lengths unless given as (picks, wins)) -> (rect_out [B][stride][4], votes_out [B][stride] or None); asserts that the
    inputs come back unchanged and that the guard tails are untouched."""
    picks, wins = picks if isinstance(picks, tuple) else (picks, [len(p) for p in picks])
    ncols = rows.shape[1]
    assert rows.shape[0] == B * stride and len(picks) == B
    hp = np.full((B, stride), SENT, np.int64)
    for b in range(B):
        hp[b, :len(picks[b])] = picks[b]
    d = F.DeviceTensor.from_numpy(rows)
    ndev = F.DeviceTensor.from_numpy(np.asarray(counts, np.int32))
    dc = F.DeviceTensor.from_numpy(cls) if cls is not None else None
    dr = F.DeviceTensor.from_numpy(rect) if rect is not None else None
    dp = F.DeviceTensor.from_numpy(hp)
    dw = F.DeviceTensor.from_numpy(np.asarray(wins, np.int32))
    out = F.DeviceTensor.from_numpy(np.full((B * stride + 8, 4), SENT, np.float64))
    vo = F.DeviceTensor.from_numpy(np.full(B * stride + 8, SENT, np.int32)) if votes else None
    F._lib.call("frcnn_box_vote_batch", F.ptr(d), B, stride, n_cap, F.ptr(ndev), ncols, score_col, mode, C.c_float(overlap), F.ptr(dc),
                F.ptr(dr), F.ptr(dp), F.ptr(dw), F.ptr(out), F.ptr(vo), F.stream_ptr())
    out = out.numpy()
    assert np.array_equal(d.numpy().view(np.uint32), rows.view(np.uint32)), "the rows were written"
    assert ndev.numpy().tolist() == list(counts) and dw.numpy().tolist() == list(wins), "the counts were written"
    assert np.array_equal(dp.numpy(), hp), "the picks were written"
    if cls is not None:
        assert np.array_equal(dc.numpy(), cls), "the classes were written"
    if rect is not None:
        assert dr.numpy().tobytes() == rect.tobytes(), "the rects were written"
    assert np.all(out[B * stride:] == SENT)
    if votes:
        vo = vo.numpy()
        assert np.all(vo[B * stride:] == SENT)
        vo = vo[:B * stride].reshape(B, stride)
    return out[:B * stride].reshape(B, stride, 4), vo


def _check(F, rows, B, stride, n_cap, counts, picks, mode, overlap, cls, rect, tag, wins=None):
    """-> (rect_out, votes_out, the largest error / bound met, winners with more than one voter)"""
    out, vo = _run(F, rows, B, stride, n_cap, counts, picks if wins is None else (picks, wins), mode, overlap, cls, rect)
    worst, many = 0.0, 0
    for b in range(B):
        n = min(counts[b], n_cap)
        seg = slice(b * stride, b * stride + n)
        k = min(len(picks[b]) if wins is None else wins[b], n)
        p = np.asarray(picks[b][:k], np.int64)
        t = "%s segment %d (n %d, winners %d)" % (tag, b, n, k)
        want_rect, want_votes = np.full((stride, 4), SENT, np.float64), np.full(stride, SENT, np.int32)
        if k:
            own = (rect[seg] if rect is not None else rows[seg, :4].astype(np.float64))[p - 1]
            ref, votes, A = V.box_vote(rows[seg], p, overlap, 5, mode, None if cls is None else cls[seg],
                                       None if rect is None else rect[seg])
            got = out[b][p - 1]
            assert np.array_equal(vo[b][p - 1], votes), "%s: votes" % t
            single = votes < 2
            assert got[single].tobytes() == own[single].tobytes(), "%s: a winner with fewer than two voters keeps its own rect" % t
            for q in np.nonzero(~single)[0]:
                for c in range(4):
                    bound = V.rect_error_bound(int(votes[q]), A[q, c], mode)
                    err = abs(got[q, c] - ref[q, c])
                    assert err <= bound, "%s: winner %d coordinate %d: error %.3g above the bound %.3g (%d voters)" % (
                        t, p[q], c, err, bound, votes[q])
                    if bound > 0:
                        worst = max(worst, err / bound)
            many += int(np.sum(~single))
            want_rect[p - 1], want_votes[p - 1] = got, votes
        # everything outside the winners' rows still holds the sentinel
        assert out[b].tobytes() == want_rect.tobytes(), "%s: stores outside the winners' rows" % t
        assert np.array_equal(vo[b], want_votes), "%s: votes stored outside the winners' rows" % t
    return out, vo, worst, many


def _winner_sets(rng, n):
    """none, one, every row (in random order), one more than the waves of a block"""
    perm = rng.permutation(n) + 1
    return [("none", perm[:0]), ("one", perm[:1]), ("every", perm), ("waves+1", perm[:min(WAVES + 1, n)])]


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_winner_counts_against_the_restatement(F, n):
    worst, many, i = 0.0, 0, 0
    for kind in ("clustered", "disjoint"):
        for name, picks in _winner_sets(np.random.RandomState(n), n):
            mode = (V.LOG_SCORE, V.SCORE, V.UNIFORM)[i % 3]
            cmode = ("none", "three", "none", "distinct")[i % 4]
            rng = np.random.RandomState(100 * n + i)
            rows = np.concatenate([_inputs(kind, 7 * n + i, n, mode), np.full((3, 5), 9.0, np.float32)])   # (rows past the count)
            cls = _classes(cmode, rng, len(rows))
            rect = _rects(rng, rows) if i % 2 else None
            _, _, w, m = _check(F, rows, 1, len(rows), n, [n], [picks], mode, MANY, cls, rect,
                                "%s n=%d %s mode %d cls=%s" % (kind, n, name, mode, cmode))
            worst, many, i = max(worst, w), many + m, i + 1
    print("n = %d: %d winners with more than one voter, largest error / bound %.3f" % (n, many, worst))
    assert n < 3 or many > 0, "no winner has two voters: the means are not exercised"


@pytest.mark.parametrize("n", [257, LDS_ROWS + 1])
def test_weight_modes_classes_and_rects(F, n):
    """every weight mode x (no classes, three classes, all distinct) x (rect NULL, fp64 rects that differ from the boxes)"""
    worst = 0.0
    for mode in (V.UNIFORM, V.SCORE, V.LOG_SCORE):
        rows = _inputs("clustered", n + mode, n, mode)
        for ci, cmode in enumerate(("none", "three", "distinct")):
            for given in (False, True):
                rng = np.random.RandomState(10 * n + 3 * mode + ci)
                cls = _classes(cmode, rng, n)
                rect = _rects(rng, rows) if given else None
                picks = (rng.permutation(n) + 1)[:min(n, 300)]
                _, vo, w, many = _check(F, rows, 1, n, n, [n], [picks], mode, MANY, cls, rect,
                                        "n=%d mode %d cls=%s rect=%s" % (n, mode, cmode, given))
                worst = max(worst, w)
                if cmode == "distinct":
                    assert many == 0 and np.all(vo[0][picks - 1] == 1), "rows of distinct classes vote for themselves alone"
                else:
                    assert many > 0
    print("n = %d: largest error / bound %.3f" % (n, worst))


def test_the_threshold_includes_its_own_value(F):
    """[0,0,9,9] and [0,0,9,4] overlap by exactly 0.5: a vote at overlap = 0.5, none one fp32 step above"""
    rows = rows5(np.array([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32), [0.5, 0.5])
    out, vo = _run(F, rows, 1, 2, 2, [2], [np.array([1, 2])], V.SCORE, 0.5)
    assert vo[0].tolist() == [2, 2] and out[0].tolist() == [[0.0, 0.0, 9.0, 6.5]] * 2
    out, vo = _run(F, rows, 1, 2, 2, [2], [np.array([1, 2])], V.SCORE, float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert vo[0].tolist() == [1, 1] and out[0].tolist() == rows[:, :4].tolist()
    # weights 1 : 3
    rows = rows5(np.array([[0, 0, 9, 9], [2, 0, 11, 9]], np.float32), [0.25, 0.75])
    out, vo = _run(F, rows, 1, 2, 2, [2], [np.array([1])], V.SCORE, 0.5)
    assert vo[0].tolist() == [2, SENT] and out[0][0].tolist() == [1.5, 0.0, 10.5, 9.0]


@pytest.mark.parametrize("n", [65, LDS_ROWS + 1])
def test_plain_scores_that_are_no_weights_never_vote(F, n):
    """weight_mode 1 with scores 0, -0, negative, inf and NaN among good ones: such rows never vote (they may win); a segment
    of zeros returns every winner's own rect with votes = 0"""
    rng = np.random.RandomState(n)
    boxes = clustered_boxes(rng, n, per=24)
    sc = rng.choice(np.array([0.0, -0.0, -0.5, np.inf, np.nan, 0.3, 0.7, 0.9], np.float32), n)
    rows = rows5(boxes, sc)
    rows[:, 4] = sc
    picks = (rng.permutation(n) + 1)[:min(n, 300)]
    for cls in (None, _classes("three", rng, n)):
        _, vo, _, many = _check(F, rows, 1, n, n, [n], [picks], V.SCORE, MANY, cls, _rects(rng, rows), "bad scores n=%d" % n)
        assert many > 0
        bad = ~(np.isfinite(sc) & (sc > 0))
        assert np.any(bad[picks - 1]) and np.any(vo[0][picks - 1][bad[picks - 1]] != 1), "a winner that does not vote itself"
    zeros = rows5(boxes, np.zeros(n, np.float32))
    rect = _rects(rng, zeros)
    out, vo, _, many = _check(F, zeros, 1, n, n, [n], [picks], V.SCORE, MANY, None, rect, "zeros n=%d" % n)
    assert many == 0 and np.all(vo[0][picks - 1] == 0) and out[0][picks - 1].tobytes() == rect[picks - 1].tobytes()


SEGMENTS = {1: ([299], [50]),
            3: ([0, 300, 307], [3, 0, 40]),                       # an empty segment, count = 0 in the middle, a count above n_cap
            8: ([300, 63, 0, 307, 1, 129, 200, 65], [40, 70, 4, 0, 1, 5, 200, 9])}   # (63 rows, 70 winners announced: all 63 win)


@pytest.mark.parametrize("B", sorted(SEGMENTS))
@pytest.mark.parametrize("cmode", ["none", "three"])
def test_segments_with_unequal_counts(F, B, cmode):
    n_cap, stride = 300, 311
    counts, wins = SEGMENTS[B]
    many = 0
    for mode in (V.UNIFORM, V.SCORE, V.LOG_SCORE):
        rng = np.random.RandomState(50 + 10 * B + mode)
        rows = np.full((B * stride, 5), 9.0, np.float32)
        for b in range(B):
            rows[b * stride:b * stride + n_cap] = _inputs("disjoint" if b % 3 == 1 else "clustered", 100 * B + 10 * b + mode, n_cap, mode)
        cls = _classes(cmode, rng, B * stride)
        rect = _rects(rng, rows) if mode != V.SCORE else None
        # every segment offers picks -- also the empty one and the one whose count is 0: nothing may be stored for them
        picks = [(rng.permutation(max(min(counts[b], n_cap), 1)) + 1)[:max(wins[b], 4)] for b in range(B)]
        _, _, _, m = _check(F, rows, B, stride, n_cap, counts, picks, mode, MANY, cls, rect, "B=%d mode %d cls=%s" % (B, mode, cmode),
                            wins=wins)
        many += m
    assert many > 0


def test_result_depends_on_the_segment_alone(F):
    """the same segment in slot 0 of B = 1 and in slot 2 of B = 3, each run twice: bit-identical rects and votes (both tiers)"""
    for n, mode in ((300, V.LOG_SCORE), (LDS_ROWS + 1, V.SCORE)):
        stride = n + 5
        rng = np.random.RandomState(n)
        seg = np.concatenate([_inputs("clustered", n, n, mode), np.full((5, 5), 9.0, np.float32)])
        cls, rect = _classes("three", rng, stride), _rects(rng, seg)
        picks = (rng.permutation(n) + 1)[:200]
        runs = []
        for rep in range(2):
            o1, v1 = _run(F, seg, 1, stride, n, [n], [picks], mode, MANY, cls, rect)
            other = [np.concatenate([_inputs("clustered", n + 1 + b, n, mode), np.full((5, 5), 9.0, np.float32)]) for b in range(2)]
            rows3 = np.concatenate(other + [seg])
            cls3 = np.concatenate([_classes("three", rng, stride), _classes("three", rng, stride), cls])
            rect3 = np.concatenate([_rects(rng, other[0]), _rects(rng, other[1]), rect])
            o3, v3 = _run(F, rows3, 3, stride, n, [n - 7, n, n], [picks[:50][picks[:50] <= n - 7], picks[:9], picks], mode, MANY,
                          cls3, rect3)
            runs.append((o1[0], v1[0], o3[2], v3[2]))
        o, v = runs[0][0], runs[0][1]
        assert np.any(v[picks - 1] > 1)
        for o1, v1, o3, v3 in runs:
            assert o1.tobytes() == o.tobytes() and o3.tobytes() == o.tobytes(), n
            assert np.array_equal(v1, v) and np.array_equal(v3, v), n


def test_argument_errors_launch_nothing_and_store_nothing(F):
    rows = F.DeviceTensor.zeros((64, 5), np.float32)
    i = F.DeviceTensor.from_numpy(np.full(64, 16, np.int32))
    p = F.DeviceTensor.from_numpy(np.arange(1, 65, dtype=np.int64))
    out = F.DeviceTensor.from_numpy(np.full((64, 4), SENT, np.float64))
    vo = F.DeviceTensor.from_numpy(np.full(64, SENT, np.int32))
    f = C.c_float
    good = dict(boxes=F.ptr(rows), B=1, stride=16, n_cap=16, n_dev=F.ptr(i), ncols=5, score_col=5, weight_mode=1, overlap=f(0.5),
                cls=None, rect=None, pick=F.ptr(p), count=F.ptr(i), rect_out=F.ptr(out), votes_out=F.ptr(vo))
    bad = [dict(B=0), dict(B=-1), dict(n_cap=-1), dict(stride=15), dict(ncols=3, weight_mode=0), dict(score_col=4), dict(score_col=6),
           dict(score_col=4, weight_mode=2), dict(score_col=6, weight_mode=2), dict(ncols=4, score_col=4), dict(weight_mode=3),
           dict(weight_mode=-1), dict(overlap=f(0.0)), dict(overlap=f(-0.5)), dict(overlap=f(1.5)), dict(overlap=f(float("nan"))),
           dict(boxes=None), dict(n_dev=None), dict(pick=None), dict(count=None), dict(rect_out=None)]

    def call(args):
        F._lib.call("frcnn_box_vote_batch", *(list(args.values()) + [F.stream_ptr()]))

    def errors():
        for t in bad:
            with pytest.raises(F.FrcnnError):
                call(dict(good, **t))
    la = _launches(F, errors)
    assert sum(la.values()) == 0, la
    assert np.all(out.numpy() == SENT) and np.all(vo.numpy() == SENT), "an argument error stored something"
    # the counter does count, under the per-class pass's class; votes_out may be NULL; uniform weights take 4 columns and any score_col
    la = _launches(F, lambda: (call(good), call(dict(good, votes_out=None)), call(dict(good, weight_mode=0, score_col=0)),
                               call(dict(good, n_cap=0, stride=0))))
    assert la["nms"] == 3 and sum(la.values()) == 3, la         # (n_cap = 0: nothing to launch)
    # (16 coincident rows: no voter under the zero scores of the first call, 16 under the uniform weights of the third)
    assert np.all(vo.numpy()[:16] == 16) and np.all(vo.numpy()[16:] == SENT) and not out.numpy()[:16].any()


def test_python_surface(F):
    n = 300
    rng = np.random.RandomState(4)
    cls = _classes("three", rng, n)
    picks = (rng.permutation(n) + 1)[:60]
    for weights, mode in (("score", V.SCORE), ("log_score", V.LOG_SCORE), ("uniform", V.UNIFORM)):
        rows = _inputs("clustered", 11 + mode, n, mode)
        rect = _rects(rng, rows)
        for classes, rects in ((None, None), (cls, rect)):
            ref, votes, A = V.box_vote(rows, picks, MANY, 5, mode, classes, rects)
            dev = lambda a: None if a is None else F.DeviceTensor.from_numpy(a)
            for args in ((rows, picks, classes, rects), (dev(rows), dev(picks), dev(classes), dev(rects))):
                r, v = F.box_vote(args[0], args[1], MANY, 5, weights, classes=args[2], rects=args[3])
                assert r.dtype == np.float64 and r.shape == (60, 4) and v.dtype == np.int32 and np.array_equal(v, votes)
                assert votes.max() > 1
                for q in range(60):
                    for c in range(4):
                        assert abs(r[q, c] - ref[q, c]) <= V.rect_error_bound(int(votes[q]), A[q, c], mode), (weights, q, c)
    r, v = F.box_vote(rows, picks[:0])
    assert r.shape == (0, 4) and v.shape == (0,)
    # the picks of nms() are winners as they come
    keep = F.nms(rows, 0.3, 5)
    r, v = F.box_vote(rows, keep, 0.3, weights="uniform")
    assert r.shape == (len(keep), 4) and np.array_equal(v, V.box_vote(rows, keep, 0.3, 5, V.UNIFORM)[1])
    for bad in (np.array([0]), np.array([n + 1])):
        with pytest.raises(ValueError):
            F.box_vote(rows, bad)


# ------------------------------------------------------------------------------------------------ Detector level
# 0.1: the per-class pass deletes what overlaps a winner by more than 0.1, so whatever it deletes votes for a winner (the first
# NMS has already thinned the candidates at 0.25: overlaps of 0.5 between survivors are rare in any frame)
VOTING = dict(score=dict(overlap=0.1), uniform=dict(overlap=0.1, weight="uniform"))


def _vote_collect(F, d, frames):
    """_collect, plus what the record holds under voting, per frame"""
    out = []
    for f in frames:
        r = _collect(d, [f])[0]
        rec = d._last
        for k in ("bb", "kc", "r2", "keep_row", "votes"):
            if k in rec:
                r[k] = rec[k].copy()
        out.append(r)
    return out


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
    for name, t in VOTING.items():
        s[name] = _vote_collect(F, F.Detector(model, box_voting=t), frames)
    print("box voting: survivors %s, winners %s, votes of the winners %s"
          % ([r["kept"] for r in s["plain"]], [r["nwin"] for r in s["plain"]],
             [sorted(r["votes"][r["votes"] > 0].tolist(), reverse=True)[:6] if "votes" in r else [] for r in s["score"]]))
    return s


def test_key_absent_changes_nothing_and_launches_nothing_new(F, setup):
    s = setup
    got = {}

    def run(name, d):
        def fn():
            got[name] = _collect(d, s["frames"])
            got[name + "/batch"] = d.detect_batch(s["frames"])
            got[name + "/records"] = d.last_batch
        return _launches(F, fn)
    plain = F.Detector(s["model"])
    la0 = run("plain", plain)
    assert plain.box_voting is None and not [k for k in plain._bufs if "voted" in k or "votes" in k], "nothing new is allocated"
    la1 = run("none", F.Detector(s["model"], box_voting=None))
    m = dict(s["model"], cfg=dict(s["cfg"], box_voting=None))
    la2 = run("cfg none", F.Detector(m))
    assert la0 == la1 == la2, "the same launches per kernel class"
    for name in ("plain", "none", "cfg none"):
        _same(got[name], s["plain"], name)
        for b in range(len(SEEDS)):
            assert _winner_rows(got[name + "/batch"][b]) == s["plain"][b]["winners"], (name, b)
            for k in ("bb", "kc", "r2", "keep_row", "votes"):
                assert k not in got[name + "/records"][b], (name, b, k)
    d = F.Detector(s["model"], box_voting={})
    assert d.box_voting == (0.5, "score")
    la3 = _launches(F, lambda: _collect(d, s["frames"]))
    busy = sum(r["n"] > 0 and len(r["pick"]) > 0 for r in s["plain"])
    assert la3["nms"] - busy == _launches(F, lambda: _collect(F.Detector(s["model"]), s["frames"]))["nms"] and busy > 0
    # the cfg's key is read when the call names none, and the call's table wins
    m = dict(s["model"], cfg=dict(s["cfg"], box_voting=dict(weight="uniform")))
    assert F.Detector(m).box_voting == (0.5, "uniform") and F.Detector(m, box_voting=dict(overlap=0.3)).box_voting == (0.3, "score")


def _rows_of(r):
    """the survivor row (0-based) of every winner of a frame: keep_row is the survivors' candidate position"""
    pos = dict((int(c) + 1, j) for j, c in enumerate(r["keep_row"].tolist()))
    return np.array([pos[w[1]] for w in _winner_keys(r["winners"])], np.int64)


@pytest.mark.parametrize("name", sorted(VOTING))
def test_winners_keep_everything_but_r2_and_r2_is_the_restatement(F, setup, name):
    s = setup
    overlap, mode = VOTING[name]["overlap"], (V.UNIFORM if name == "uniform" else V.LOG_SCORE)
    voted = moved = 0
    worst = 0.0
    for b, (r, p) in enumerate(zip(s[name], s["plain"])):
        tag = "%s frame %d" % (name, b)
        assert r["n"] == p["n"] and r["kept"] == p["kept"] and np.array_equal(r["pick"], p["pick"]) and r["nwin"] == p["nwin"], tag
        # identity, order and every field except r2 (columns 9:13 of _winner_rows' tuples)
        assert [w[:9] + w[13:] for w in r["winners"]] == [w[:9] + w[13:] for w in p["winners"]], tag
        if r["n"] == 0 or len(r["pick"]) == 0:
            assert "bb" not in r and r["nwin"] == 0
            continue
        K = r["kept"]
        assert r["bb"].shape == (K, 5) and r["kc"].shape == (K,) and r["r2"].shape == (K, 4) and r["r2"].dtype == np.float64
        assert r["keep_row"].shape == (K,) and r["votes"].shape == (K,) and r["votes"].dtype == np.int32
        if r["nwin"] == 0:
            continue
        rows = _rows_of(r)
        assert [int(r["kc"][j]) for j in rows] == [w[0] for w in _winner_keys(r["winners"])], tag
        # without the key a winner's r2 is its row of the record's (unvoted) r2
        assert [w[9:13] for w in p["winners"]] == [tuple(r["r2"][j].tolist()) for j in rows], tag
        ref, votes, A = V.box_vote(r["bb"], rows + 1, overlap, 5, mode, r["kc"], r["r2"])
        assert np.array_equal(r["votes"][rows], votes), "%s: votes" % tag
        rest = np.ones(K, bool)
        rest[rows] = False
        assert not r["votes"][rest].any(), "%s: votes of rows that did not win" % tag
        for q, w in enumerate(r["winners"]):
            got = np.array(w[9:13])
            if votes[q] < 2:
                assert got.tobytes() == r["r2"][rows[q]].tobytes(), "%s winner %d: fewer than two voters" % (tag, q)
                continue
            voted += 1
            moved += got.tobytes() != r["r2"][rows[q]].tobytes()
            for c in range(4):
                bound = V.rect_error_bound(int(votes[q]), A[q, c], mode)
                err = abs(got[c] - ref[q, c])
                assert err <= bound, "%s winner %d coordinate %d: error %.3g above the bound %.3g" % (tag, q, c, err, bound)
                worst = max(worst, err / bound)
    print("%s: %d winners with more than one voter (%d moved), largest error / bound %.3f" % (name, voted, moved, worst))
    assert voted > 0 and moved > 0, "no winner of the fixture has votes > 1: nothing is exercised"


@pytest.mark.parametrize("combo", ["voting", "voting+gaussian+score"])
def test_detect_batch_equals_the_detect_loop_under_voting(F, setup, combo):
    s = setup
    kw = dict(box_voting=VOTING["score"])
    if combo != "voting":
        kw.update(nms=dict(method="gaussian"), proposals=dict(order="score", pre_nms_top_n=50))
    want = _vote_collect(F, F.Detector(s["model"], **kw), s["frames"])
    assert any("votes" in r and r["votes"].size and r["votes"].max() > 1 for r in want)
    for batch in (8, 3):
        d = F.Detector(s["model"], **kw)
        d.BATCH = batch
        res = d.detect_batch(s["frames"])
        for b, (rec, win, w) in enumerate(zip(d.last_batch, res, want)):
            tag = "%s BATCH %d frame %d" % (combo, batch, b)
            assert _winner_rows(win) == w["winners"], tag
            assert rec["n"] == w["n"] and rec["kept"] == w["kept"] and np.array_equal(rec["pick"], w["pick"]), tag
            for k in ("bb", "kc", "r2", "keep_row", "votes"):      # (also of the frames whose chunk's buffers were reused: detach())
                assert (k in rec) == (k in w), (tag, k)
                if k in w:
                    assert rec[k].dtype == w[k].dtype and rec[k].tobytes() == w[k].tobytes(), (tag, k)
    if combo != "voting":
        # the votes are weighed by the UNDECAYED confidences: bb is the class test's output, whatever the soft pass did to the scores
        plain = _vote_collect(F, F.Detector(s["model"], box_voting=VOTING["score"], proposals=kw["proposals"]), s["frames"])
        for w, p in zip(want, plain):
            if "bb" in w:
                assert w["bb"].tobytes() == p["bb"].tobytes()
    res = F.Detector(s["model"], **kw).detect_batch(s["frames"], shared_cnet=True)
    assert sum(len(x) for x in res) > 0


def test_evaluate_detections_in_batches_at_two_thresholds(F, setup):
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import evaluate_detections
    s = setup
    d = F.Detector(s["model"], box_voting=VOTING["score"])
    items = []
    for img in s["frames"][:6]:
        rois = []
        for j, x in enumerate(list(d.detect(img))[::3]):
            r = x["r2"]
            rois.append(F.Roi(Rect(r.minX, r.minY, r.maxX, r.maxY) if j % 2 == 0 else r.offset(r.width() * 0.3, 0), x["class"]))
        rois.append(F.Roi(Rect(5, 5, 40, 40), 16))
        items.append(dict(img=img, rois=rois))
    one = evaluate_detections(F.Detector(s["model"], box_voting=VOTING["score"]), _Val(items), len(items), batch=1,
                              iou_threshold=(0.5, 0.75))
    print("tp at 0.5: %d, at 0.75: %d" % (one["by_iou"][0.5]["tp"], one["by_iou"][0.75]["tp"]))
    assert sorted(one["by_iou"]) == [0.5, 0.75] and one["detections"] > 0 and one["by_iou"][0.5]["tp"] >= one["by_iou"][0.75]["tp"] > 0
    assert one["mAP"] == (one["by_iou"][0.5]["mAP"] + one["by_iou"][0.75]["mAP"]) / 2
    four = evaluate_detections(F.Detector(s["model"], box_voting=VOTING["score"]), _Val(items), len(items), batch=4,
                               iou_threshold=(0.5, 0.75))
    assert four == one
