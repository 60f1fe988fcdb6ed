"""Problems for frcnn_rpn_scan_ragged (frames of different sizes in one call), no GPU and no library: ONE anchor-table pair for
every frame (the tables do not depend on the image size), per frame its own head-map sizes and its own image size, and one of
the patterns none / all / random, built the way anchor_ops_ref.scan_case builds its frames:

  none    no anchor passes the threshold test (an empty frame)
  all     every anchor passes it and its rect lies around the image's centre (a full frame: count == anchors)
  random  half of the anchors pass it; 40 % of those are put just inside or just outside one of the image's four borders (the kinds
          in rotation), the others keep random regression values -- the image sizes are small beside the anchor tables (centres
          up to a few hundred pixels), so many of those rects miss the image: both outcomes of the overlap test

The input conditions (tests/test_scan_ragged_host.py): no anchor of any frame has exp(c1) within anchor_ops_ref.MARGIN of the
threshold or an overlap distance under MARGIN of the image's size, so membership is decided identically by every correct fp64
evaluation and no anchor has to be left out of a comparison."""
import functools

import numpy as np

import anchor_ops_ref as ref

THR = ref.THR
# head-map sizes (H, W) per layer
SIZES = {
    "n12": [(1, 1)] * 4,
    "n72": [(3, 5), (2, 3), (1, 2), (1, 1)],
    "n1026": [(14, 11), (9, 10), (7, 12), (2, 7)],       # two anchors in the compaction's second 1024-chunk
    "n2490": [(23, 17), (15, 13), (11, 14), (9, 10)],    # three chunks, the last one partial
    "n1287": [(200, 1), (1, 200), (3, 5), (2, 7)],       # the last row of the 200-entry tables, in y and in x
}
PATTERNS = ("none", "all", "random")
# the frames: (sizes, pattern, (img_w, img_h)); every size with "random", the smallest and the largest with every pattern
FRAMES = (
    ("n12", "all", (300.0, 200.0)), ("n12", "none", (64.0, 48.0)), ("n12", "random", (90.0, 140.0)),
    ("n72", "random", (120.0, 90.0)), ("n72", "all", (64.0, 48.0)),
    ("n1026", "random", (90.0, 140.0)), ("n1026", "all", (120.0, 90.0)), ("n1026", "none", (300.0, 200.0)),
    ("n2490", "random", (210.0, 160.0)), ("n2490", "none", (120.0, 90.0)), ("n2490", "all", (90.0, 140.0)),
    ("n1287", "random", (300.0, 200.0)), ("n1287", "all", (210.0, 160.0)),
)
# the calls of the GPU test, as indices into FRAMES
CALL_B3 = (5, 8, 3)                                          # the largest frame in the middle
CALL_B17 = tuple([0, 1, 3, 4, 2, 6][i % 6] for i in range(17))   # crosses the 16-frame launch group; small frames cycled
CALL_TRUNCATED = (3, 6)                                      # cap = 5; the second frame is "all"
ONE_SIZE = ("n1026", (90.0, 140.0))                          # B frames of one size: the three patterns


def total(name):
    return 3 * sum(h * w for h, w in SIZES[name])


@functools.lru_cache(maxsize=None)
def tables():
    return ref.anchor_tables(np.random.RandomState(4242))


@functools.lru_cache(maxsize=None)
def frame(name, pattern, img):
    """-> dict(maps: four fp32 [18][H][W], H, W, img_w, img_h, total, want: scan_ref's result, flags, pattern, name)"""
    img_w, img_h = img
    sizes = SIZES[name]
    H = [h for h, w in sizes]
    W = [w for h, w in sizes]
    aw, ah = tables()
    n_all = total(name)
    rng = np.random.RandomState(11 + 31 * PATTERNS.index(pattern) + 1009 * sorted(SIZES).index(name) + int(img_w) + 7 * int(img_h))
    flags = ref.scan_pattern(pattern, n_all, rng)
    v = np.zeros((n_all, 6))
    v[:, 0] = np.where(flags, 30.0, -30.0)
    v[:, 1] = rng.uniform(-5.0, 25.0, n_all)

    def draw(n):
        return np.concatenate([rng.randn(n, 2) * 0.5, rng.randn(n, 2) * 0.3], 1)
    v[:, 2:] = draw(n_all)
    border = np.full(n_all, -1)
    on = np.nonzero(flags)[0]
    at_border = pattern == "random"
    chosen = on[rng.rand(on.size) < 0.4] if at_border else on
    aw64, ah64 = aw.astype(np.float64), ah.astype(np.float64)
    all_idx = ref._all_idx(H, W)
    for j, n in enumerate(chosen):
        l, a, y, x = all_idx[n]
        x0, x1 = aw64[l, a, x]
        y0, y1 = ah64[l, a, y]
        tx, ty = (img_w / 2 - x0) / (x1 - x0), (img_h / 2 - y0) / (y1 - y0)     # the other axis: well inside
        if not at_border:
            border[n] = ref.BORDER_CENTRE
            v[n, 2:4] = (tx, ty)
            continue
        kind = j % 8
        side, inside = kind // 2, kind % 2
        border[n] = kind
        d = ref.BORDER if inside else -ref.BORDER
        if side == 0:
            tx = (img_w - d - x0) / (x1 - x0)
        elif side == 1:
            tx = (-(x1 - x0) + d - x0) / (x1 - x0)
        elif side == 2:
            ty = (img_h - d - y0) / (y1 - y0)
        else:
            ty = (-(y1 - y0) + d - y0) / (y1 - y0)
        v[n, 2:] = (tx, ty, 0.0, 0.0)
    # an anchor of the random share that came to lie within the margin of a border is drawn again
    for _ in range(20):
        maps = ref._to_maps(v, H, W)
        want = ref.scan_ref(maps, H, W, aw, ah, img_w, img_h, THR)
        bad = np.nonzero((want["ovl_margin"].min(1) < 4 * ref.MARGIN) & (border < 0))[0]
        if bad.size == 0:
            break
        v[bad, 2:] = draw(bad.size)
    return dict(name=name, pattern=pattern, maps=maps, H=H, W=W, img_w=img_w, img_h=img_h, want=want, flags=flags, border=border,
                total=n_all)


def frames(indices=None):
    return [frame(*FRAMES[i]) for i in (range(len(FRAMES)) if indices is None else indices)]


def one_size_frames():
    return [frame(ONE_SIZE[0], p, ONE_SIZE[1]) for p in PATTERNS]
