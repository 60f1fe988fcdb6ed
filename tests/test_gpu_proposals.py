"""Score-ordered proposals with pre- and post-NMS caps (cfg.proposals).  Kernel level: frcnn_topk_select against numpy's
lexsort on value-compared keys, frcnn_rpn_gather_rows against fancy indexing -- identities.  Detector level (vgg_small, amplified
weights, 128x176 frames): the settings off change nothing and launch nothing new; a cap that cuts nothing equals no cap; the
capped, score-ordered frame equals the numpy selection of the uncapped scan, the oracle's NMS on the device's own rows, and a
host recomposition of the winners from the device's own arrays; detect_batch equals the detect() loop under every setting."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_detect_batch import _amplified_weights, _frames, _winner_rows

pytestmark = pytest.mark.gpu
SENTINEL = -7
NS = [0, 1, 63, 64, 65, 1000, 26544, 45015]


# ------------------------------------------------------------------------------------------------ kernel level: selection
def _unique(rng, n):
    return (-(rng.permutation(n) + 1.0) / (n + 1.0) * 0.05).astype(np.float32)


def _quantised(rng, n):
    return (rng.randint(0, 8, n) * -0.00625).astype(np.float32)


def _equal(rng, n):
    return np.full(n, -0.01, np.float32)


def _zeros_block(rng, n):
    """the saturated log-softmax case: a block of exact 0.0 among negatives, mixed with -0.0"""
    p = (-rng.rand(n) * 0.05 - 1e-6).astype(np.float32)
    z = rng.rand(n) < 0.4
    p[z] = 0.0
    p[z & (rng.rand(n) < 0.5)] = -0.0
    return p


def _one_inf(rng, n):
    p = _unique(rng, n)
    if n:
        p[rng.randint(n)] = -np.inf
    return p


def _one_nan(rng, n):
    p = _quantised(rng, n)
    if n:
        p[rng.randint(n)] = np.nan
    return p


SCORES = dict(unique=_unique, quantised=_quantised, equal=_equal, zeros=_zeros_block, inf=_one_inf, nan=_one_nan)


def _want(p, K):
    """the K best-ranked rows, ascending: value-compared keys (-0 == +0, a NaN sorts behind everything), ties by the lower row"""
    rows = np.arange(len(p))
    return np.sort(np.lexsort((rows, -p))[:K])


def _select(F, score, B, stride, n_cap, counts, K):
    """frcnn_topk_select on host arrays -> (sel [B][sel_stride] + guard tail, k [B] + guard entry, sel_stride); asserts that
    the inputs come back unchanged."""
    L = F._lib.load()
    sel_stride = max(min(n_cap, K), 1) + 5
    ds = F.DeviceTensor.from_numpy(score)
    ndev = F.DeviceTensor.from_numpy(np.asarray(counts, np.int32))
    sel = F.DeviceTensor.from_numpy(np.full(B * sel_stride + 64, SENTINEL, np.int32))
    k = F.DeviceTensor.from_numpy(np.full(B + 1, SENTINEL, np.int32))
    wsb = L.frcnn_topk_select_workspace_bytes(B, n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    F._lib.call("frcnn_topk_select", F.ptr(ds), B, stride, n_cap, F.ptr(ndev), K, F.ptr(sel), sel_stride, F.ptr(k), F.ptr(ws), wsb,
                F.stream_ptr())
    sel, k = sel.numpy(), k.numpy()
    assert np.array_equal(ds.numpy().view(np.uint32), score.view(np.uint32)), "the scores were written"
    assert ndev.numpy().tolist() == list(counts), "the counts were written"
    assert k[B] == SENTINEL and np.all(sel[B * sel_stride:] == SENTINEL)
    return sel, k, sel_stride


def _check_segments(F, score, B, stride, n_cap, counts, K, tag):
    sel, k, ss = _select(F, score, B, stride, n_cap, counts, K)
    for b in range(B):
        n = min(counts[b], n_cap)
        want = _want(score[b * stride:b * stride + n], K)
        kp = int(k[b])
        assert kp == min(n, K) == len(want), "%s segment %d: K' = %d" % (tag, b, kp)
        seg = sel[b * ss:(b + 1) * ss]
        assert np.array_equal(seg[:kp], want), "%s segment %d (n %d, K %d)" % (tag, b, n, K)
        assert np.all(seg[kp:] == SENTINEL), "%s segment %d: stray stores behind its rows" % (tag, b)


@pytest.mark.parametrize("kind", sorted(SCORES))
def test_topk_select_one_segment_against_numpy(F, kind):
    rng = np.random.RandomState(sorted(SCORES).index(kind))
    for n in NS:
        p = SCORES[kind](rng, n)
        n_cap = max(n, 1)
        score = np.concatenate([p, np.full(n_cap - n + 3, 9.0, np.float32)])     # (rows past the count would win if they were read)
        for K in sorted(set(k for k in (1, 64, 300, 6000, n, n + 1) if k >= 1)):
            _check_segments(F, score, 1, len(score), n_cap, [n], K, "%s n=%d K=%d" % (kind, n, K))


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("kind", sorted(SCORES))
def test_topk_select_segments_against_numpy(F, kind, B):
    """an empty segment, a full one and one whose device count exceeds n_cap in the same call"""
    rng = np.random.RandomState(100 + 10 * B + sorted(SCORES).index(kind))
    for n_cap in (65, 1000, 26544):
        counts = [0, n_cap, n_cap + 7, 63, 1, 64, n_cap // 2, 65][:B]
        stride = n_cap + 11
        score = np.full(B * stride, 9.0, np.float32)
        for b in range(B):
            score[b * stride:b * stride + n_cap] = SCORES[kind](rng, n_cap)
        for K in (1, 64, 300, 6000, n_cap, n_cap + 1):
            _check_segments(F, score, B, stride, n_cap, counts, K, "%s B=%d n_cap=%d K=%d" % (kind, B, n_cap, K))


def test_topk_select_does_not_depend_on_the_segment_slot(F):
    """the same keys in every segment: the same rows in every segment"""
    rng = np.random.RandomState(5)
    n, B, K = 5000, 8, 777
    p = _zeros_block(rng, n)
    sel, k, ss = _select(F, np.tile(p, B), B, n, n, [n] * B, K)
    for b in range(B):
        assert int(k[b]) == K and np.array_equal(sel[b * ss:b * ss + K], _want(p, K)), b


def test_topk_select_argument_errors(F):
    d = F.DeviceTensor.zeros((64,), np.float32)
    i = F.DeviceTensor.zeros((64,), np.int32)
    ws = F.DeviceTensor.empty((4096,), np.uint8)
    for args in ((F.ptr(d), 1, 8, 16, F.ptr(i), 4, F.ptr(i), 4, F.ptr(i), F.ptr(ws), 4096),      # stride < n_cap
                 (F.ptr(d), 1, 16, 16, F.ptr(i), 0, F.ptr(i), 4, F.ptr(i), F.ptr(ws), 4096),     # K < 1
                 (F.ptr(d), 1, 16, 16, F.ptr(i), 8, F.ptr(i), 4, F.ptr(i), F.ptr(ws), 4096),     # sel_stride < min(n_cap, K)
                 (F.ptr(d), 1, 16, 16, F.ptr(i), 4, F.ptr(i), 4, F.ptr(i), F.ptr(ws), 16)):      # workspace too small
        with pytest.raises(F.FrcnnError):
            F._lib.call("frcnn_topk_select", *(args + (F.stream_ptr(),)))


# ------------------------------------------------------------------------------------------------ kernel level: gather
def _gather(F, src, B, src_stride, src_rows, sel, sel_stride, kdev, k_cap, dst_stride, only_box5=False):
    dev = {k: F.DeviceTensor.from_numpy(v) for k, v in src.items()}
    dsel = F.DeviceTensor.from_numpy(sel) if sel is not None else None
    dk = F.DeviceTensor.from_numpy(np.asarray(kdev, np.int32))
    rows = B * dst_stride + 16
    out = dict(p=np.full(rows, SENTINEL, np.float32), idx=np.full((rows, 4), SENTINEL, np.int32),
               rect=np.full((rows, 4), SENTINEL, np.float64), box=np.full((rows, 4), SENTINEL, np.float32),
               box5=np.full((rows, 5), SENTINEL, np.float32), row=np.full(rows, SENTINEL, np.int32))
    o = {k: F.DeviceTensor.from_numpy(v) for k, v in out.items()}

    def dst(k):
        return None if only_box5 and k != "box5" else F.ptr(o[k])
    F._lib.call("frcnn_rpn_gather_rows", F.ptr(dev["p"]), None if only_box5 else F.ptr(dev["idx"]),
                None if only_box5 else F.ptr(dev["rect"]), F.ptr(dev["box"]), B, src_stride, src_rows, F.ptr(dsel), sel_stride, F.ptr(dk),
                k_cap, dst("p"), dst("idx"), dst("rect"), dst("box"), dst("box5"), dst("row"), dst_stride, F.stream_ptr())
    for k, v in src.items():
        assert np.array_equal(dev[k].numpy().view(np.uint8), v.view(np.uint8)), "source %s was written" % k
    return {k: v.numpy() for k, v in o.items()}


def _match_arrays(rng, rows):
    p = (-rng.rand(rows) * 0.05).astype(np.float32)
    p[::7] = -0.0
    return dict(p=p, idx=rng.randint(1, 200, (rows, 4)).astype(np.int32), rect=rng.randn(rows, 4) * 300.0,
                box=(rng.randn(rows, 4) * 300.0).astype(np.float32))


def test_gather_rows_against_fancy_indexing(F):
    rng = np.random.RandomState(9)
    B, src_stride, src_rows, k_cap = 3, 1200, 1100, 300
    sel_stride, dst_stride = k_cap + 3, k_cap + 9
    src = _match_arrays(rng, B * src_stride)
    ks = [0, k_cap, k_cap + 50]          # empty, full, and a device count above k_cap
    sel = np.full(B * sel_stride, 10 ** 6, np.int32)          # (rows past a segment's count are out of range: never used)
    for b in range(B):
        sel[b * sel_stride:b * sel_stride + k_cap] = np.sort(rng.permutation(src_rows)[:k_cap])
    got = _gather(F, src, B, src_stride, src_rows, sel, sel_stride, ks, k_cap, dst_stride)
    for k in got:
        assert np.all(got[k][B * dst_stride:] == SENTINEL), k
    for b in range(B):
        kk = min(ks[b], k_cap)
        r = sel[b * sel_stride:b * sel_stride + kk].astype(np.int64) + b * src_stride
        d = slice(b * dst_stride, b * dst_stride + kk)
        for k in ("p", "idx", "rect", "box"):
            assert np.array_equal(got[k][d].view(np.uint8), src[k][r].view(np.uint8)), "segment %d: %s" % (b, k)
            assert np.all(got[k][b * dst_stride + kk:(b + 1) * dst_stride] == SENTINEL), "segment %d: stray stores in %s" % (b, k)
        want5 = np.concatenate([src["box"][r], src["p"][r][:, None]], 1)
        assert np.array_equal(got["box5"][d].view(np.uint32), want5.view(np.uint32)), "segment %d: box5" % b
        assert np.array_equal(got["row"][d], r - b * src_stride + 1), "segment %d: row" % b
        assert np.all(got["box5"][b * dst_stride + kk:(b + 1) * dst_stride] == SENTINEL)
        assert np.all(got["row"][b * dst_stride + kk:(b + 1) * dst_stride] == SENTINEL)


def test_gather_rows_without_a_selection_builds_box5_only(F):
    rng = np.random.RandomState(10)
    B, stride = 2, 700
    src = _match_arrays(rng, B * stride)
    ks = [0, 650]
    got = _gather(F, src, B, stride, stride, None, 0, ks, stride, stride, only_box5=True)
    for k in ("p", "idx", "rect", "box", "row"):
        assert np.all(got[k] == SENTINEL), k
    want5 = np.concatenate([src["box"], src["p"][:, None]], 1)
    assert np.all(got["box5"][:stride] == SENTINEL)
    assert np.array_equal(got["box5"][stride:stride + 650].view(np.uint32), want5[stride:stride + 650].view(np.uint32))
    assert np.all(got["box5"][stride + 650:] == SENTINEL)


# ------------------------------------------------------------------------------------------------ Detector level
H, W = 128, 176
SEEDS = list(range(5, 13))
M_POST = 20


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
    s["y2"] = _collect(F.Detector(model), frames)
    s["score"] = _collect(F.Detector(model, proposals=dict(order="score")), frames)
    ns = [r["n"] for r in s["y2"]]
    print("proposals: matches %s, candidates (y2) %s, (score) %s, winners (score) %s"
          % (ns, [len(r["pick"]) for r in s["y2"]], [len(r["pick"]) for r in s["score"]], [r["nwin"] for r in s["score"]]))
    # what the tests below lean on
    assert sum(n >= 64 for n in ns) >= 4, "fewer than 4 of the 8 frames have 64 matches"
    assert any(len(np.unique(r["p"])) < r["n"] for r in s["y2"]), "no frame has two matches of equal p"
    assert any(len(r["pick"]) > M_POST for r in s["score"]), "no frame has more than M candidates"
    return s


def _collect(d, frames):
    """[everything detect(f) leaves behind] per frame, from Detector d"""
    out = []
    for f in frames:
        win = d.detect(f)
        m = d.last_scan
        out.append(dict(n=m["n"], idx=m["idx"].numpy(), p=m["p"].numpy(), rect=m["rect"].numpy(), box=m["box"].numpy(),
                        row=m["row"].numpy() if "row" in m else None, matches=m.get("matches"),
                        pick=d.last_pick.copy(), cnet=d.last_cnet if m["n"] else None, kept=d._last.get("kept", 0),
                        winners=_winner_rows(win), nwin=len(win)))
    return out


def _same(got, want, what, rows=True):
    assert len(got) == len(want)
    for b, (g, r) in enumerate(zip(got, want)):
        tag = "%s frame %d" % (what, b)
        assert g["n"] == r["n"], tag
        for k in ("idx", "p", "rect", "box", "pick") + (("row",) if rows else ()):
            if r[k] is None:
                assert g[k] is None, "%s: %s" % (tag, k)
            else:
                assert g[k].dtype == r[k].dtype and g[k].shape == r[k].shape and np.array_equal(g[k], r[k]), "%s: %s" % (tag, k)
        if rows:
            assert g["matches"] == r["matches"], tag
        if r["cnet"] is None:
            assert g["cnet"] is None, tag
        else:
            for k in ("bbox", "cls"):
                assert np.array_equal(g["cnet"][k], r["cnet"][k]), "%s: cnet %s" % (tag, k)
        assert g["kept"] == r["kept"] and g["winners"] == r["winners"], tag


def _launches(F, fn):
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return {n: la[i] for i, n in enumerate(F._lib.KC_NAMES)}


def test_settings_off_change_nothing_and_launch_nothing_new(F, setup):
    s = setup
    got = {}

    def run(name, d):
        def fn():
            got[name] = _collect(d, s["frames"])
            got[name + "/batch"] = d.detect_batch(s["frames"])
            got[name + "/records"] = d.last_batch
        return _launches(F, fn)
    la0 = run("default", F.Detector(s["model"]))
    la1 = run("y2", F.Detector(s["model"], proposals=dict(order="y2")))
    assert la0["topk"] == 0 and la1["topk"] == 0
    assert la0 == la1, "the same launches per kernel class"
    _same(got["default"], s["y2"], "default")
    _same(got["y2"], s["y2"], "{order = y2}")
    for b in range(len(SEEDS)):
        assert _winner_rows(got["y2/batch"][b]) == _winner_rows(got["default/batch"][b]) == s["y2"][b]["winners"]
        assert "row" not in got["y2/records"][b] and np.array_equal(got["y2/records"][b]["pick"], s["y2"][b]["pick"])
    # (the counter does count: one selection and one gather a frame under a cap, one gather a frame under order = "score")
    la2 = _launches(F, lambda: _collect(F.Detector(s["model"], proposals=dict(pre_nms_top_n=50)), s["frames"]))
    la3 = _launches(F, lambda: _collect(F.Detector(s["model"], proposals=dict(order="score")), s["frames"]))
    assert la2["topk"] == 2 * len(SEEDS) and la3["topk"] == len(SEEDS)


@pytest.mark.parametrize("order", ["y2", "score"])
def test_a_cap_that_cuts_nothing_equals_no_cap(F, setup, order):
    s = setup
    ns = [r["n"] for r in s[order]]
    for K in (max(ns), 10 ** 6):         # (max(ns): K == n for one frame, K > n for the others)
        d = F.Detector(s["model"], proposals=dict(order=order, pre_nms_top_n=K))
        got = _collect(d, s["frames"])
        _same(got, s[order], "%s K=%d" % (order, K), rows=False)
        for g in got:
            assert g["matches"] == g["n"] and np.array_equal(g["row"], np.arange(1, g["n"] + 1))


def _recompose(F, O, d, R):
    """the winners of the frame Detector d has just processed, from the DEVICE'S OWN arrays: the class test on last_cnet
    (Detector.lua:110-115), then per class nms(bb, 0.1) keyed by the confidence column on the device's bb rows
    -> [(class, candidate row 1-based)] classes ascending, pick order within a class"""
    logp = d.last_cnet["cls"]
    bg = d.model["cfg"]["class_count"] + 1
    cls = np.argmax(logp, axis=1) + 1
    conf = logp[np.arange(len(cls)), cls - 1]
    keep = np.nonzero((cls != bg) & (np.exp(conf.astype(np.float64)) > 0.2))[0]
    kept = d._last["kept"]
    assert kept == len(keep)
    bb = d._buf("bb", (R, 5)).numpy()[:kept]
    kc = d._buf("kc", (R,), np.int32).numpy()[:kept]
    keep_row = d._buf("keep_row", (R,), np.int32).numpy()[:kept]
    assert np.array_equal(keep_row, keep) and np.array_equal(kc, cls[keep]) and np.array_equal(bb[:, 4], conf[keep])
    want = []
    for c in sorted(set(kc.tolist())):
        rows = np.nonzero(kc == c)[0]
        for i in O.nms(bb[rows], 0.1, 2, 5).tolist():
            want.append((c, int(keep_row[rows[i - 1]]) + 1))
    return want


def test_score_order_under_a_cap_identities(F, O, setup):
    s = setup
    d = F.Detector(s["model"])
    deep = 0
    for b, f in enumerate(s["frames"]):
        ref = s["score"][b]                     # the uncapped scan of the frame
        n = ref["n"]
        for K in sorted(set(k for k in (1, n // 2, n - 1) if k >= 1)):
            d.set_proposals(dict(order="score", pre_nms_top_n=K))
            win = d.detect(f)
            m = d.last_scan
            rows = _want(ref["p"], K)
            assert m["n"] == len(rows) == min(n, K) and m["matches"] == n
            assert np.array_equal(m["row"].numpy(), rows + 1), "frame %d K %d: selected rows" % (b, K)
            for k in ("p", "idx", "rect", "box"):
                assert np.array_equal(m[k].numpy().view(np.uint8), ref[k][rows].view(np.uint8)), "frame %d K %d: %s" % (b, K, k)
            box5 = np.concatenate([ref["box"][rows], ref["p"][rows][:, None]], 1)
            assert d.last_pick.tolist() == O.nms(box5, 0.25, 2, 5).tolist(), "frame %d K %d: picks" % (b, K)
            want = _recompose(F, O, d, len(d.last_pick))
            assert [(x["class"], x["candidate"]) for x in win] == want, "frame %d K %d: winners" % (b, K)
            for x in win:        # a winner's anchor data are those of its candidate's SELECTED row
                i = int(d.last_pick[x["candidate"] - 1]) - 1
                assert x["p"] == float(ref["p"][rows[i]]) and x["l"] == int(ref["idx"][rows[i]][0])
            deep += len(win) > 0
    assert deep > 0, "no capped frame had winners"


def test_y2_order_under_a_cap_keeps_the_reference_nms(F, O, setup):
    s = setup
    d = F.Detector(s["model"])
    for b, f in enumerate(s["frames"]):
        ref = s["y2"][b]
        K = max(ref["n"] // 2, 1)
        d.set_proposals(dict(pre_nms_top_n=K))
        d.detect(f)
        rows = _want(ref["p"], K)
        assert np.array_equal(d.last_scan["row"].numpy(), rows + 1)
        assert np.array_equal(d.last_scan["box"].numpy(), ref["box"][rows])
        assert d.last_pick.tolist() == O.nms(ref["box"][rows], 0.25).tolist()


def test_post_nms_top_n_keeps_the_first_picks(F, O, setup):
    s = setup
    d = F.Detector(s["model"], proposals=dict(order="score", post_nms_top_n=M_POST))
    cut = 0
    for b, f in enumerate(s["frames"]):
        ref = s["score"][b]
        win = d.detect(f)
        R = len(ref["pick"])
        assert d.last_pick.tolist() == ref["pick"][:min(R, M_POST)].tolist(), "frame %d" % b
        assert d.last_cnet["cls"].shape[0] == min(R, M_POST)
        assert [(x["class"], x["candidate"]) for x in win] == _recompose(F, O, d, min(R, M_POST)), "frame %d: winners" % b
        cut += R > M_POST
    assert cut > 0


def _settings(setup):
    ns = sorted(r["n"] for r in setup["y2"])
    k_mix = ns[len(ns) // 2 - 1]            # some frames above it, some not
    assert ns[0] <= k_mix < ns[-1]
    return [dict(order="score"), dict(order="score", pre_nms_top_n=10 ** 6), dict(order="y2", pre_nms_top_n=10 ** 6),
            dict(order="score", pre_nms_top_n=k_mix), dict(order="y2", pre_nms_top_n=k_mix), dict(order="score", pre_nms_top_n=1),
            dict(order="score", post_nms_top_n=M_POST), dict(order="score", pre_nms_top_n=k_mix, post_nms_top_n=M_POST)]


def _records(d):
    out = []
    for r in d.last_batch:
        out.append(dict(n=r["n"], idx=r["idx"], p=r["p"], rect=r["rect"], box=r["box"], pick=r["pick"], cnet=r["cnet"], kept=r["kept"],
                        row=r["row"] if "row" in r else None, matches=r["matches"] if "matches" in r else None))
    return out


def test_detect_batch_equals_the_detect_loop_under_every_setting(F, setup):
    s = setup
    for t in _settings(s):
        want = _collect(F.Detector(s["model"], proposals=t), s["frames"])
        d = F.Detector(s["model"], proposals=t)
        res = d.detect_batch(s["frames"])
        got = _records(d)
        for g, w in zip(got, res):
            g["winners"] = _winner_rows(w)
        _same(got, want, str(t))
        if "pre_nms_top_n" in t and t["pre_nms_top_n"] < 10 ** 6 and t["pre_nms_top_n"] > 1:
            cut = [g["matches"] > g["n"] for g in got]
            assert any(cut) and not all(cut), "the chunk does not mix frames above and below K"
        # a second call of three frames on the same Detector: the records of the first call have been detached
        res2 = d.detect_batch(s["frames"][:3])
        assert [_winner_rows(w) for w in res2] == [r["winners"] for r in want[:3]], str(t)


def test_shared_cnet_keeps_working_under_the_settings(F, setup):
    """one classification-net pass per chunk: everything up to the picks is bit-identical to the detect() loop, the net's
    outputs agree within its own error (the 1e-3 bar of test_gpu_detect_batch), the candidate counts are the clamped ones"""
    from util import assert_close
    s = setup
    t = _settings(s)[-1]
    want = _collect(F.Detector(s["model"], proposals=t), s["frames"])
    d = F.Detector(s["model"], proposals=t)
    d.detect_batch(s["frames"], shared_cnet=True)
    for b, (g, w) in enumerate(zip(_records(d), want)):
        for k in ("n", "matches"):
            assert g[k] == w[k]
        for k in ("idx", "p", "rect", "box", "pick", "row"):
            assert np.array_equal(g[k], w[k]), "frame %d: %s" % (b, k)
        assert len(g["pick"]) <= M_POST
        for k in ("bbox", "cls"):
            assert_close(g["cnet"][k], w["cnet"][k], 1e-3, "frame %d: cnet %s of the shared pass" % (b, k))


def test_proposals_are_the_candidates_detect_used(F, setup):
    s = setup
    for t in (None, dict(order="score", pre_nms_top_n=100, post_nms_top_n=M_POST),
              dict(order="score", pre_nms_top_n=50, post_nms_top_n=10)):
        d = F.Detector(s["model"], proposals=t)
        for f in s["frames"][:3]:
            props = d.proposals(f)
            pick, p_scan = d.last_pick.copy(), d.last_scan["p"].numpy()
            d.detect(f)
            assert np.array_equal(d.last_pick, pick) and len(props) == len(pick) > 0
            m = d.last_scan
            p, idx, rect = m["p"].numpy(), m["idx"].numpy(), m["rect"].numpy()
            assert np.array_equal(p.view(np.uint32), p_scan.view(np.uint32))     # one first stage behind both
            for x, i in zip(props, (pick - 1).tolist()):
                assert x["p"] == float(p[i]) and x["l"] == int(idx[i][0])
                assert (x["r"].minX, x["r"].minY, x["r"].maxX, x["r"].maxY) == tuple(rect[i].tolist())
                a = d.anchors.get(*[int(v) for v in idx[i]])
                assert (x["a"].layer, x["a"].aspect, repr(x["a"].index)) == (a.layer, a.aspect, repr(a.index))
