"""frcnn_cnet_loss_rows on the device against the numpy restatement of tests/cnet_loss_ref.py, on sentinel-filled buffers with
guard rows.  Where a row involves no exp / expm1 / pow (NLL, smoothed NLL, SmoothL1, every special value) the comparison is of
bytes; elsewhere it is within the bounds derived in cnet_loss_ref.py.  Nothing is stored behind row R, the scoring mode writes
no gradient and leaves crout alone, and a refused call launches and writes nothing."""
import ctypes as C

import numpy as np
import pytest

import anchor_ops_ref as A
import cnet_loss_ref as L

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 3          # rows behind row R in every output


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


def _desc(F, d, ncls):
    from frcnn_amd.objective import cnet_loss_desc
    return cnet_loss_desc(d, ncls)


def launch(F, c, d, train=True, want=("row_loss", "key", "box5"), desc=None, **bad):
    """one call on fresh sentinel outputs -> (rc, dict of host copies with their guard rows, launches per kernel class).
    arg_NAME = value replaces the good argument NAME."""
    R, ncls, npos = c["R"], c["ncls"], c["npos"]
    n = max(R, 1)
    dev = dict((k, F.DeviceTensor.from_numpy(np.ascontiguousarray(c[k]) if R else np.zeros((1,) + c[k].shape[1:], c[k].dtype)))
               for k in ("crout", "crtarget", "ccout", "cctarget", "roi"))
    out = dict(crdelta=_sent(F, (n + GUARD, 4), np.float32), ccdelta=_sent(F, ((n + GUARD) * ncls,), np.float32),
               row_loss=_sent(F, (n + GUARD, 2), np.float64), key=_sent(F, (n + GUARD,), np.float32),
               box5=_sent(F, (n + GUARD, 5), np.float32))
    desc = _desc(F, d, ncls) if desc is None else desc
    a = dict(crout=F.ptr(dev["crout"]), crtarget=F.ptr(dev["crtarget"]), ccout=F.ptr(dev["ccout"]), cctarget=F.ptr(dev["cctarget"]),
             roi=F.ptr(dev["roi"]), R=R, npos=npos, ncls=ncls, desc=C.byref(desc),
             crdelta=F.ptr(out["crdelta"]) if train else None, ccdelta=F.ptr(out["ccdelta"]) if train else None,
             row_loss=F.ptr(out["row_loss"]) if "row_loss" in want else None, key=F.ptr(out["key"]) if "key" in want else None,
             box5=F.ptr(out["box5"]) if "box5" in want else None)
    a.update((k[4:], v) for k, v in bad.items())
    rc, la = _profiled(F, lambda: F._lib.load().frcnn_cnet_loss_rows(
        a["crout"], a["crtarget"], a["ccout"], a["cctarget"], a["roi"], a["R"], a["npos"], a["ncls"], a["desc"], a["crdelta"], a["ccdelta"],
        a["row_loss"], a["key"], a["box5"], F.stream_ptr()))
    host = dict((k, v.numpy()) for k, v in out.items())
    host["crout"] = dev["crout"].numpy()
    return rc, host, la


def _close(dev, ref, tol, what):
    """finite reference values within tol; the others (inf, NaN) the same value"""
    dev = np.asarray(dev, np.float64); ref = np.asarray(ref, np.float64); tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(dev[~fin], ref[~fin], equal_nan=True), what + ": special values"
    diff = np.abs(dev[fin] - ref[fin])
    bad = diff > tol[fin]
    assert not bad.any(), "%s: %d values off, worst %g against a bound of %g" % (what, bad.sum(), diff[bad].max(), tol[fin][bad].min())


def check(F, c, d, exact, train=True):
    R, ncls, npos = c["R"], c["ncls"], c["npos"]
    rc, got, la = launch(F, c, d, train=train)
    assert rc == 0
    assert sum(la) == la[F._lib.KC_NAMES.index("elemwise")] == 1
    ref = L.loss_ref(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], npos, d, roi=c["roi"], train=train)
    # ---- nothing behind row R; the scoring mode writes no gradient and leaves crout alone
    for k in ("crdelta", "row_loss", "key", "box5"):
        assert _is_sent(got[k][R:]), "behind row R of " + k
    assert _is_sent(got["ccdelta"][R * ncls:]), "behind row R of ccdelta"
    if not train:
        assert _is_sent(got["crdelta"]) and _is_sent(got["ccdelta"])
        assert got["crout"].tobytes() == np.ascontiguousarray(c["crout"]).tobytes()
    else:
        assert got["crout"].tobytes() == ref["crout"].tobytes()
    ccd = got["ccdelta"][:R * ncls].reshape(R, ncls)
    bw = d["box_weight"]
    err = ref["err"]
    if exact:
        assert not err["cls"].any() and not err["box"].any()
        if train:
            assert got["crdelta"][:R].tobytes() == ref["crdelta"].tobytes() and ccd.tobytes() == ref["ccdelta"].tobytes()
        assert got["key"][:R].tobytes() == ref["key"].tobytes() and got["box5"][:R].tobytes() == ref["box5"].tobytes()
        assert np.array_equal(got["row_loss"][:R], ref["row_loss"], equal_nan=True)
    else:
        if train:
            _close(got["crdelta"][:R], ref["crdelta"], L.spacing32(ref["crdelta"]) + err["crdelta"], "crdelta")
            tgt = np.zeros((R, ncls), bool)
            valid = (c["cctarget"] >= 1) & (c["cctarget"] <= ncls)
            tgt[np.nonzero(valid)[0], c["cctarget"][valid].astype(np.int64) - 1] = True
            assert not ccd[~tgt].any() and not ref["ccdelta"][~tgt].any()
            _close(ccd, ref["ccdelta"], L.spacing32(ref["ccdelta"]) + err["gt"][:, None], "ccdelta")
        e_box = bw * err["box"] + L.ULP * np.abs(ref["row_loss"][:, 0])
        e_cls = err["cls"] + L.ULP * np.abs(ref["cls"])
        _close(got["row_loss"][:R, 0], ref["row_loss"][:, 0], e_box, "row_loss: box")
        _close(got["row_loss"][:R, 1], ref["row_loss"][:, 1], e_cls / R, "row_loss: cls")
        _close(got["key"][:R], ref["key"], L.spacing32(ref["key"]) + e_box + e_cls, "key")
        assert got["box5"][:R, :4].tobytes() == ref["box5"][:, :4].tobytes() and got["box5"][:R, 4].tobytes() == got["key"][:R].tobytes()
    assert not np.isnan(got["key"][:R]).any()
    return got, ref


@pytest.mark.parametrize("R,ncls,npos", L.SHAPES)
def test_rows_equal_the_restatement(F, R, ncls, npos):
    """every description on one shape, with the labelled edge cases planted (cnet_loss_ref.edge_rows), in the training mode and --
    keys only -- in the scoring mode"""
    for name in L.DESCS:
        c, lab, d = L.case(R, ncls, npos, name)
        got, ref = check(F, c, d, name in L.EXACT, train=True)
        score, _ = check(F, c, d, name in L.EXACT, train=False)
        for k in ("key", "box5", "row_loss"):        # one arithmetic: the two modes give the same bits
            assert score[k].tobytes() == got[k].tobytes(), (name, k)
        for r in lab.get("bad_target", []):
            assert got["key"][r] == -np.inf and np.isnan(got["row_loss"][r, 1]) and not got["ccdelta"][r * ncls:(r + 1) * ncls].any()
        for r in lab.get("nan_input", []):
            assert got["key"][r] == np.inf
        if d["box"] == "giou":
            for r in lab.get("giou_equal", []):     # exactly zero: loss and gradient
                assert got["row_loss"][r, 0] == 0.0 and not got["crdelta"][r].any()
            for r in lab.get("giou_above_K", []):
                assert not got["crdelta"][r, 2:].any()
            if d["box_weight"] == 0.0:
                assert not got["crdelta"][:R].any() and not got["row_loss"][:R, 0].any()


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_focal_at_probability_one(F, gamma):
    """lp = 0 on every row: q = 0, and neither the loss nor the gradient is anything but zero (no 0 * inf from q^(gamma - 1))"""
    c = L.random_rows(5, 65, 3, 1)
    c["ccout"][np.arange(65), c["cctarget"].astype(np.int64) - 1] = 0.0
    d = L.desc(cls="focal", gamma=gamma, box_weight=0.0)
    got, _ = check(F, c, d, False)
    assert not got["ccdelta"][:65 * 3].any() and not got["row_loss"][:65, 1].any() and not got["key"][:65].any()


@pytest.mark.parametrize("R", [1, 63, 65, 257])
def test_default_desc_is_frcnn_cnet_losses(F, R):
    """the defaults against the parent's kernel on the same inputs: crdelta, ccdelta and the zeroed crout bit for bit; the
    accumulated pair within one fp32 unit of the parent's (it rounds each sum to fp32 once; the box sum before its factor 10) plus
    frcnn_loss_accumulate's stated bound"""
    for ncls in (2, 17):
        for npos in A.cnet_npos(R):
            a = A.cnet_losses_case(R, npos, ncls)
            c = dict(crout=a["crout"], crtarget=a["crtarget"], ccout=a["ccout"], cctarget=a["cctarget"], roi=np.zeros((R, 4)), R=R,
                     ncls=ncls, npos=npos)
            rc, got, _ = launch(F, c, L.DEFAULT)
            assert rc == 0
            crout = F.DeviceTensor.from_numpy(a["crout"]); crdelta = _sent(F, (R, 4), np.float32); ccdelta = _sent(F, (R, ncls), np.float32)
            d_in = [F.DeviceTensor.from_numpy(a[k]) for k in ("crtarget", "ccout", "cctarget")]
            loss2 = F.DeviceTensor.zeros((2,), np.float64); acc = F.DeviceTensor.zeros((2,), np.float64)
            F._lib.call("frcnn_cnet_losses", crout.ptr, F.ptr(d_in[0]), F.ptr(d_in[1]), F.ptr(d_in[2]), R, npos, ncls, crdelta.ptr, ccdelta.ptr,
                        loss2.ptr, F.stream_ptr())
            assert got["crdelta"][:R].tobytes() == crdelta.numpy().tobytes()
            assert got["ccdelta"][:R * ncls].tobytes() == ccdelta.numpy().tobytes()
            assert got["crout"].tobytes() == crout.numpy().tobytes()
            rl = F.DeviceTensor.from_numpy(np.ascontiguousarray(got["row_loss"][:R]))
            F._lib.call("frcnn_loss_accumulate", rl.ptr, R, acc.ptr, F.stream_ptr())
            mine, parent = acc.numpy(), loss2.numpy()
            (w0, w1), (b0, b1) = L.accumulate_ref(got["row_loss"][:R])
            assert (mine[0], mine[1]) == (w0, w1)                         # the accumulate's order is the stated one
            own = 8 * 2.0 ** -53 * np.abs(got["row_loss"][:R]).sum(0)
            assert abs(mine[0] - parent[0]) <= 10.0 * float(np.spacing(np.float32(abs(parent[0]) / 10.0))) + b0 + own[0]
            assert abs(mine[1] - parent[1]) <= float(np.spacing(np.float32(abs(parent[1])))) + b1 + own[1]


def test_two_runs_give_the_same_bits(F):
    c, _, d = L.case(300, 21, 300, "focal1_giou")
    _, a, _ = launch(F, c, d)
    _, b, _ = launch(F, c, d)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_outputs_are_optional_one_by_one(F):
    c, _, d = L.case(65, 17, 1, "smoothed")
    _, full, _ = launch(F, c, d)
    for want in (("key",), ("row_loss",), ("box5",), ()):
        rc, got, _ = launch(F, c, d, train=True, want=want)
        assert rc == 0
        for k in ("key", "row_loss", "box5"):
            assert (got[k].tobytes() == full[k].tobytes()) if k in want else _is_sent(got[k]), (want, k)
        assert got["ccdelta"].tobytes() == full["ccdelta"].tobytes() and got["crdelta"].tobytes() == full["crdelta"].tobytes()
    rc, got, la = launch(F, dict(c, R=0, npos=0), d)              # no rows: no launch
    assert rc == 0 and sum(la) == 0 and all(_is_sent(got[k]) for k in ("crdelta", "ccdelta", "row_loss", "key", "box5"))


def test_refusals_leave_the_sentinels_intact(F):
    c, _, d = L.case(65, 17, 1, "default")
    good = _desc(F, d, 17)

    def mod(**kw):
        m = F._lib.CnetLossDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    off = F.DeviceTensor.empty((64,), np.float32)
    bad_calls = [dict(arg_R=-1), dict(arg_npos=-1), dict(arg_npos=66), dict(arg_ncls=0), dict(arg_crout=None), dict(arg_crtarget=None),
                 dict(arg_ccout=None), dict(arg_cctarget=None), dict(arg_desc=None), dict(arg_crdelta=None), dict(arg_ccdelta=None),
                 dict(arg_roi=None), dict(arg_crout=C.c_void_p(off.ptr + 4)), dict(arg_crtarget=C.c_void_p(off.ptr + 8)),
                 dict(arg_crdelta=C.c_void_p(off.ptr + 4)), dict(arg_ccdelta=C.c_void_p(off.ptr + 12)), dict(arg_roi=C.c_void_p(off.ptr + 8))]
    bad_descs = [mod(cls=2), mod(cls=-1), mod(box=2), mod(gamma=-0.5), mod(gamma=5.5), mod(gamma=float("nan")), mod(alpha=0.0), mod(alpha=1.0),
                 mod(alpha=float("nan")), mod(alpha=0.5, bgclass=0), mod(alpha=0.5, bgclass=18), mod(smoothing=1.0), mod(smoothing=-0.1),
                 mod(cls=1, smoothing=0.1), mod(beta=0.0), mod(beta=float("inf")), mod(beta=float("nan")), mod(box_weight=-1.0),
                 mod(box_weight=float("inf"))]
    runs = [launch(F, c, d, **b) for b in bad_calls] + [launch(F, c, d, desc=m) for m in bad_descs]
    runs.append(launch(F, c, d, train=False, want=()))            # no output at all
    for i, (rc, got, la) in enumerate(runs):
        assert rc != 0 and sum(la) == 0, i
        assert all(_is_sent(got[k]) for k in ("crdelta", "ccdelta", "row_loss", "key", "box5")), i
        assert got["crout"].tobytes() == np.ascontiguousarray(c["crout"]).tobytes(), i
    assert "cnet_loss_rows" in F._lib.load().frcnn_last_error().decode()


def test_host_wrapper(F):
    """nms.cnet_loss: the kernel on host arrays, with the sums of frcnn_loss_accumulate"""
    c, _, d = L.case(65, 17, 65, "focal1_giou")
    st = dict((k, v) for k, v in d.items() if v is not None)
    res = F.cnet_loss(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], st, roi=c["roi"])
    _, got, _ = launch(F, c, d)
    assert res["key"].tobytes() == got["key"][:65].tobytes() and res["box5"].tobytes() == got["box5"][:65].tobytes()
    assert res["crdelta"].tobytes() == got["crdelta"][:65].tobytes() and res["ccdelta"].tobytes() == got["ccdelta"][:65 * 17].tobytes()
    want, _ = L.accumulate_ref(res["row_loss"])
    assert np.array_equal(np.array(res["loss"]), np.array(want), equal_nan=True)
    score = F.cnet_loss(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], st, train=False)
    assert "crdelta" not in score and "box5" not in score and score["key"].tobytes() == res["key"].tobytes()
    with pytest.raises(F.FrcnnError, match="cnet_loss"):
        F.cnet_loss(c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["npos"], dict(cls="focal", label_smoothing=0.5))
