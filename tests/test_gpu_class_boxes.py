"""frcnn_detect_class_boxes_batch (csrc/class_boxes.hip) on host arrays, through class_boxes() of the package: the box of its own
class for every row of an all-class class test.  Against three references, none of which looks at the kernel under test:
  * the device's own pieces -- frcnn_box_head_forward (kind 1) on the gathered feature rows for the deltas and frcnn_detect_post
    for their decode: the WHOLE output (r2, bb) bit for bit, rows behind K, column 5 and other frames' rows included (sentinel
    fill).  A wrong delta, a wrong anchor or a copy of the decode that rounds differently fails here;
  * the numpy restatement (tests/class_boxes_ref.py): x0 and y0 of r2 bit for bit, x1 and y1 within decode_bound (the two exp()
    are different libraries, each within an ulp), bb[0..3] == float32(r2); on integer-valued data everything exactly;
  * the float64 product: the deltas within box_head_ref.forward_bound at the case's nf.
Shapes: nf on both sides of a wave's 64 floats, the scalar path (nf % 4 != 0) and the vector path; 1, 3 and 17 classes; 1 and 3
frames with features at non-zero, non-monotone row0; 0, 1, 5 and 67 candidates (67 rows: more than one workgroup, a tail); K at
0, mid, row_stride and above it; classes 0 and C + 1 among the rows."""
import ctypes as C

import numpy as np
import pytest

import box_head_ref as BH
import class_boxes_ref as R

pytestmark = pytest.mark.gpu

_cache = {}


def _ks(B, cands):
    """the K pattern of a case: three frames run mid / over / zero; one frame runs the pattern its candidate count picks"""
    if B > 1:
        return ("mid", "over", "zero")
    return {1: ("mid",), 5: ("full",), 67: ("over",)}.get(cands, ("zero",))


def _device_pieces(F, P):
    """per frame (deltas fp32 k x 4 from frcnn_box_head_forward kind 1 on the gathered rows, r2 fp64 k x 4 and boxes fp32 k x 4
    of them from frcnn_detect_post: class 1 at confidence 0 for all, background 2, threshold 0.5 -- every row is kept, in order)"""
    out = []
    for b in range(P["B"]):
        k = min(int(P["K"][b]), P["row_stride"])
        if k == 0:
            out.append((np.zeros((0, 4), np.float32), np.zeros((0, 4)), np.zeros((0, 4), np.float32)))
            continue
        r, c = P["keep_row"][b, :k], P["kc"][b, :k]
        d = F.box_head(P["feat"][P["row0"][b] + r], P["W"], P["b"], classes=c.astype(np.int32), n_fg=k)["out"]
        dev = [F.DeviceTensor.from_numpy(a) for a in (np.ones(k, np.int32), np.zeros(k, np.float32), d, P["rect"][b],
                                                       P["pick"][b][r].astype(np.int64))]
        bb, kc, kr = F.DeviceTensor.empty((k, 5)), F.DeviceTensor.empty((k,), np.int32), F.DeviceTensor.empty((k,), np.int32)
        r2, K = F.DeviceTensor.empty((k, 4), np.float64), F.DeviceTensor.empty((1,), np.int32)
        F._lib.call("frcnn_detect_post", *([F.ptr(t) for t in dev] + [k, 2, 0.5] + [F.ptr(t) for t in (bb, kc, kr, r2, K)]
                                          + [F.stream_ptr()]))
        assert int(K.numpy()[0]) == k
        out.append((d, r2.numpy().copy(), bb.numpy()[:, :4].copy()))
    return out


def _case(F, nf, Cn, B, cands, integer=False):
    key = (nf, Cn, B, cands, integer)
    if key not in _cache:
        P = R.problem(R.case_seed(nf, Cn, B, cands), nf, Cn, B, cands, integer=integer, Ks=_ks(B, cands))
        got = F.class_boxes(P["feat"], P["row0"], P["W"], P["b"], P["rect"], P["pick"], P["kc"], P["keep_row"], P["K"], P["bb"], P["r2"])
        _cache.clear()          # (one case at a time: the references are shared by the asserts of a case, not kept for the run)
        _cache[key] = (P, got, _device_pieces(F, P))
    return _cache[key]


def _expected(P, pieces):
    bb, r2 = P["bb"].copy(), P["r2"].copy()
    for b, (_, q, box) in enumerate(pieces):
        k = len(q)
        r2[b, :k] = q
        bb[b, :k, :4] = box
    return bb, r2


@pytest.mark.parametrize("cands", R.CANDS)
@pytest.mark.parametrize("B", R.FRAMES)
@pytest.mark.parametrize("Cn", R.CLASSES)
@pytest.mark.parametrize("nf", R.NF)
def test_rows_get_the_box_of_their_class(F, nf, Cn, B, cands):
    P, got, pieces = _case(F, nf, Cn, B, cands)
    tag = "nf %d C %d B %d cands %d" % (nf, Cn, B, cands)
    assert got["code"] == 0, tag
    # the problem is the one the docstring promises
    assert min(P["row0"]) > 0 and (B == 1 or list(P["row0"]) != sorted(P["row0"])), tag
    if cands >= 5:
        rows = [c for f in P["per"] for cl in f for c in cl]
        assert 0 in rows or Cn + 1 in rows, tag
        assert any(len(cl) > 1 for f in P["per"] for cl in f), tag
        assert not np.array_equal(P["pick"][0][:cands], np.arange(1, cands + 1)), tag
    # 1. the whole output against the device's own pieces, bit for bit: deltas of frcnn_box_head_forward, decode of detect_post
    want_bb, want_r2 = _expected(P, pieces)
    assert got["r2"].tobytes() == want_r2.tobytes(), "%s: r2 against box_head_forward + detect_post" % tag
    assert got["bb"].tobytes() == want_bb.tobytes(), "%s: bb against box_head_forward + detect_post" % tag
    dl = R.deltas(P)
    for b, (d, q, box) in enumerate(pieces):
        k = len(d)
        assert k == dl[b][2]
        if k == 0:
            assert (got["r2"][b] == R.SENT).all() and (got["bb"][b] == np.float32(R.SENT)).all(), "%s: frame %d wrote" % (tag, b)
            continue
        g = got["r2"][b, :k]
        assert (got["r2"][b, k:] == R.SENT).all() and (got["bb"][b, k:] == np.float32(R.SENT)).all(), "%s: rows behind K" % tag
        assert (got["bb"][b, :k, 4] == np.float32(R.SENT)).all(), "%s: the confidence column" % tag
        # 2. the restated decode of those deltas: x0, y0 bit for bit; x1, y1 within the two exp()'s ulp; bb = float32(r2)
        anchor = P["rect"][b][P["pick"][b][P["keep_row"][b, :k]] - 1]
        ref, bound = R.decode(anchor, d), R.decode_bound(anchor, d)
        err = np.abs(g - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            print("%s frame %d: rows %d, decode err / bound max %.3g" % (tag, b, k, float(np.nanmax(err[:, 2:] / bound[:, 2:]))))
        assert g[:, :2].tobytes() == ref[:, :2].tobytes(), "%s: x0 / y0 against the restated decode" % tag
        assert (err <= bound).all(), "%s: x1 / y1 against the restated decode" % tag
        assert got["bb"][b, :k, :4].tobytes() == g.astype(np.float32).tobytes(), "%s: bb != float32(r2)" % tag
        # 3. the deltas against the float64 product, within the operation-count bound at this nf; no class: exactly 0
        d64, mag, _ = dl[b]
        assert (np.abs(d.astype(np.float64) - d64) <= BH.forward_bound(nf, mag)).all(), "%s: deltas" % tag
        c = P["kc"][b, :k]
        assert not d[(c < 1) | (c > Cn)].any(), "%s: a row without a class has deltas" % tag


@pytest.mark.parametrize("nf,Cn,B,cands", [(1, 3, 3, 5), (7, 17, 3, 67), (64, 3, 1, 67), (260, 17, 3, 67), (4, 1, 1, 5)])
def test_integer_data_is_exact(F, nf, Cn, B, cands):
    """small integers: every product, sum and rounding is exact in fp32 and fp64 (the extent deltas are 0: exp(0) = 1 on every
    library), so the float64 restatement is the answer bit for bit -- the indexing (row0, keep_row, pick, the class's rows)"""
    P, got, _ = _case(F, nf, Cn, B, cands, integer=True)
    want = R.class_boxes(P)
    assert got["code"] == 0
    assert got["r2"].tobytes() == want["r2"].tobytes() and got["bb"].tobytes() == want["bb"].tobytes()
    assert any(min(int(P["K"][b]), P["row_stride"]) > 0 for b in range(B))


def test_argument_errors_leave_the_outputs_untouched(F):
    P = R.problem(7, 8, 3, 3, 5)
    args = [P[k] for k in ("feat", "row0", "W", "b", "rect", "pick", "kc", "keep_row", "K", "bb", "r2")]
    for bad in (dict(B=-1), dict(B=65536), dict(nf=0), dict(C=0), dict(C=1 << 20, nf=1 << 10), dict(row_stride=-1),
                dict(match_stride=-1)):
        got = F.class_boxes(*args, overrides=bad)
        assert got["code"] != 0, bad
        assert F._lib.load().frcnn_last_error().decode().startswith("detect_class_boxes_batch"), bad
        assert got["r2"].tobytes() == P["r2"].tobytes() and got["bb"].tobytes() == P["bb"].tobytes(), bad
    neg = list(args)
    neg[1] = [P["row0"][0], -1, P["row0"][2]]
    got = F.class_boxes(*neg)
    assert got["code"] != 0 and got["r2"].tobytes() == P["r2"].tobytes() and got["bb"].tobytes() == P["bb"].tobytes()
    # nothing to do: no launch, no error, nothing written
    for none in (dict(B=0), dict(row_stride=0)):
        got = F.class_boxes(*args, overrides=none)
        assert got["code"] == 0 and got["r2"].tobytes() == P["r2"].tobytes() and got["bb"].tobytes() == P["bb"].tobytes(), none
    # NULL pointers are refused before a launch
    lib, p = F._lib.load(), C.c_void_p(0x1000)
    row0 = (C.c_longlong * 1)(0)
    full = [p, 8, row0, 1, p, p, 3, p, p, 12, p, p, p, 16, p, p, None]
    assert lib.frcnn_detect_class_boxes_batch(*[None if i == 2 else a for i, a in enumerate(full)]) != 0
    for i in (0, 4, 5, 7, 8, 10, 11, 12, 14, 15):
        assert lib.frcnn_detect_class_boxes_batch(*[None if j == i else a for j, a in enumerate(full)]) != 0, i


def test_reproducible_run_to_run(F):
    P, got, _ = _case(F, 260, 17, 3, 67)
    again = F.class_boxes(P["feat"], P["row0"], P["W"], P["b"], P["rect"], P["pick"], P["kc"], P["keep_row"], P["K"], P["bb"], P["r2"])
    assert again["r2"].tobytes() == got["r2"].tobytes() and again["bb"].tobytes() == got["bb"].tobytes()
