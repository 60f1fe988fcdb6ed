"""Test-time augmentation (cfg.tta) restated in numpy: the view list of a frame and what frcnn_detect_merge_views computes.
float64 throughout, ONE numpy operation per kernel operation (numpy does not contract a product and a sum), then
astype(float32) for the box rows -- so the comparison with the device is bit for bit."""
import numpy as np


def views(hflip, scales, H, W):
    """[(scale, flip, dH, dW)] of an H x W frame: scale-major in the order given, the unmirrored view first; the sizes truncate
    (BatchIterator.lua:52); scale 1 is the frame."""
    out = []
    for s in scales:
        dH, dW = (H, W) if float(s) == 1.0 else (max(1, int(H * float(s))), max(1, int(W * float(s))))
        out.append((float(s), False, dH, dW))
        if hflip:
            out.append((float(s), True, dH, dW))
    return out


def geometry(view_list, H, W):
    """(flip, Wv, ax, ay) per view: what the kernel takes"""
    return [(int(flip), float(dW), float(W) / dW, float(H) / dH) for _, flip, dH, dW in view_list]


def to_frame(r2, flip, Wv, ax, ay):
    """K x 4 float64 rects of a view -> the frame's coordinates: un-mirror, then the two factors (a factor of 1 is skipped)"""
    r = np.array(r2, np.float64).reshape(-1, 4).copy()
    if flip:
        a = np.float64(Wv) - r[:, 2]
        b = np.float64(Wv) - r[:, 0]
        r[:, 0], r[:, 2] = a, b
    if ax != 1.0:
        r[:, 0] = r[:, 0] * np.float64(ax)
        r[:, 2] = r[:, 2] * np.float64(ax)
    if ay != 1.0:
        r[:, 1] = r[:, 1] * np.float64(ay)
        r[:, 3] = r[:, 3] * np.float64(ay)
    return r


def merge(view_rows, geo, match_stride):
    """One frame.  view_rows: per view dict(bb K x 5 float32, kc K int32, keep_row K int32, r2 K x 4 float64, pick R int64 (1-based),
    n (its matches)); geo: geometry() -> dict(bb, kc, keep_row, r2, pick, counts = (matches, candidates, K'), roff)"""
    bb, kc, keep, r2, pick, roff = [], [], [], [], [], [0]
    for v, (rows, (flip, Wv, ax, ay)) in enumerate(zip(view_rows, geo)):
        r = to_frame(rows["r2"], flip, Wv, ax, ay)
        b = np.empty((len(r), 5), np.float32)
        b[:, :4] = r.astype(np.float32)
        b[:, 4] = np.asarray(rows["bb"], np.float32).reshape(-1, 5)[:, 4]
        bb.append(b); r2.append(r)
        kc.append(np.asarray(rows["kc"], np.int32))
        keep.append((roff[-1] + np.asarray(rows["keep_row"], np.int64)).astype(np.int32))
        pick.append(v * int(match_stride) + np.asarray(rows["pick"], np.int64))
        roff.append(roff[-1] + len(rows["pick"]))
    out = dict(bb=np.concatenate(bb), kc=np.concatenate(kc), keep_row=np.concatenate(keep), r2=np.concatenate(r2),
               pick=np.concatenate(pick), roff=np.array(roff, np.int64))
    out["counts"] = (int(sum(int(x["n"]) for x in view_rows)), int(roff[-1]), len(out["kc"]))
    return out


def view_of(candidate, roff):
    """the 0-based view of a 1-based candidate of the concatenation"""
    return int(np.searchsorted(np.asarray(roff)[:-1], candidate - 1, side="right")) - 1
