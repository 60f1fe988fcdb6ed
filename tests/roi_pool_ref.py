"""Plain numpy restatement of ROI max pooling as csrc/roi.hip states it (frcnn_roi_pool_forward / _backward), the case tables of
tests/test_gpu_roi_pool.py, and a restatement of roi.hip's launch rules that LABELS those cases.  No device code.

  forward(fmap, wins, kh, kw)           -> (out (R, C*kh*kw) float32, idx (R, C*kh*kw) int32), rows [C][kh][kw] like the device's.
                                           wins[r] = {row_lo, row_hi, col_lo, col_hi}, 1-based inclusive; cell (i, j) covers rows
                                           [i*h // kh, ceil((i+1)*h / kh)) and columns [j*w // kw, ceil((j+1)*w / kw)) of the
                                           window; the winner is the FIRST maximum in row-major order; idx = y*W + x in map
                                           coordinates
  backward(gout, idx, shape, gmap0)     -> (gmap float64, count, abs_sum): gmap = gmap0 + scatter(gout) accumulated in float64;
                                           per element of the map the number of terms of that sum and the sum of their magnitudes,
                                           gmap0 (the map the device adds into) counted as ONE term when it is given.  An idx < 0
                                           entry or a zero gout entry contributes nothing
  plan(C, H, W, R, kh, kw, det)         -> the labels of the branches of roi.hip that a forward and a backward launch of that shape
                                           take.  It only labels cases (tests/test_roi_pool_host.py checks that the tables reach
                                           every label): it is no evidence that a branch computes the right thing

Every window lies inside its map (1 <= lo <= hi <= H or W): a window outside is an out-of-bounds read on the device, so the
builder asserts it and the GPU helpers assert it again before any launch."""
import functools

import numpy as np


def cdiv(a, b):
    return -(-a // b)


def check_windows(wins, H, W):
    wins = np.asarray(wins)
    assert wins.ndim == 2 and wins.shape[1] == 4 and wins.dtype == np.int32, (wins.shape, wins.dtype)
    assert np.all(1 <= wins[:, 0]) and np.all(wins[:, 0] <= wins[:, 1]) and np.all(wins[:, 1] <= H), "a window leaves the map (rows)"
    assert np.all(1 <= wins[:, 2]) and np.all(wins[:, 2] <= wins[:, 3]) and np.all(wins[:, 3] <= W), "a window leaves the map (columns)"
    return wins


def cell_bounds(n, k):
    """[(start, end)] of the k cells along a window side of n elements"""
    return [((i * n) // k, cdiv((i + 1) * n, k)) for i in range(k)]


def forward(fmap, wins, kh, kw):
    fmap = np.asarray(fmap, np.float32)
    C, H, W = fmap.shape
    wins = check_windows(wins, H, W)
    R = len(wins)
    out = np.zeros((R, C, kh, kw), np.float32)
    idx = np.zeros((R, C, kh, kw), np.int32)
    for r, (rlo, rhi, clo, chi) in enumerate(wins.tolist()):
        r0, c0, h, w = rlo - 1, clo - 1, rhi - rlo + 1, chi - clo + 1
        xb = cell_bounds(w, kw)
        for i, (ys, ye) in enumerate(cell_bounds(h, kh)):
            for j, (xs, xe) in enumerate(xb):
                cell = fmap[:, r0 + ys:r0 + ye, c0 + xs:c0 + xe].reshape(C, -1)
                n = np.argmax(cell, axis=1)          # (the first occurrence of the maximum, in row-major order of the cell)
                out[r, :, i, j] = cell[np.arange(C), n]
                idx[r, :, i, j] = (r0 + ys + n // (xe - xs)) * W + c0 + xs + n % (xe - xs)
    return out.reshape(R, C * kh * kw), idx.reshape(R, C * kh * kw)


def backward(gout, idx, shape, gmap0=None):
    C, H, W = shape
    HW = H * W
    idx = np.asarray(idx, np.int64)
    R = idx.shape[0]
    g = np.asarray(gout, np.float64).reshape(R, C, -1)
    idx = idx.reshape(R, C, -1)
    assert g.shape == idx.shape and np.all(idx < HW)
    gmap = np.zeros(C * HW, np.float64)
    count = np.zeros(C * HW, np.int64)
    abs_sum = np.zeros(C * HW, np.float64)
    if gmap0 is not None:
        g0 = np.asarray(gmap0, np.float64).reshape(-1)
        gmap += g0
        count += 1
        abs_sum += np.abs(g0)
    live = (idx >= 0) & (g != 0.0)
    flat = (np.arange(C, dtype=np.int64)[None, :, None] * HW + idx)[live]
    np.add.at(gmap, flat, g[live])
    np.add.at(count, flat, 1)
    np.add.at(abs_sum, flat, np.abs(g[live]))
    return gmap.reshape(shape), count.reshape(shape), abs_sum.reshape(shape)


def backward_bar(count, abs_sum, det):
    """per element: the worst-case bound of an fp32 sum of n terms in any order, n 2^-23 A; in deterministic mode each term is
    rounded to a multiple of 2^-44 first (csrc/roi_fix.h): n 2^-45 more"""
    n = np.maximum(count, 1)
    return n * 2.0 ** -23 * abs_sum + (n * 2.0 ** -45 if det else 0.0)


# ---- the launch rules of roi.hip ---------------------------------------------------------------------------------------
LDS_BYTES = 64 * 1024
REQUIRED = {"cells", "generic", "idle_threads", "one_group", "channel_stride", "one_slice", "hw_lt_4",
            "lds", "atomics", "det_lds", "det_scratch"}


def forward_plan(C, H, W, R, kh, kw):
    """roi_pool_forward: the cells kernel up to 256 cells (a block of 256 threads holds `groups` channels of kh*kw cells each, the
    grid is R x slices and a thread walks the channels in steps of slices * groups), the generic kernel above"""
    cells = kh * kw
    if cells > 256:
        return {"generic"}
    labels = {"cells"}
    groups = 256 // cells
    slices = max(1, min(cdiv(C, groups), cdiv(4096, R)))
    if groups * cells < 256:
        labels.add("idle_threads")
    if groups == 1:
        labels.add("one_group")
    if slices * groups < C:
        labels.add("channel_stride")
    if slices == 1:
        labels.add("one_slice")
    if H * W < 4:
        labels.add("hw_lt_4")
    return labels


def backward_plan(H, W, det):
    """roi_pool_backward: a plane in LDS (fp32, or 64-bit fixed point in deterministic mode) while it fits into 64 KB"""
    if det:
        return {"det_lds" if H * W * 8 <= LDS_BYTES else "det_scratch"}
    return {"lds" if H * W * 4 <= LDS_BYTES else "atomics"}


def plan(C, H, W, R, kh, kw, det):
    return forward_plan(C, H, W, R, kh, kw) | backward_plan(H, W, det)


# ---- windows -----------------------------------------------------------------------------------------------------------
def edge_windows(H, W, kh, kw, seed):
    """the windows at which the kernels can go wrong, all inside the H x W map (sizes that do not fit are left out)"""
    rng = np.random.RandomState(seed)
    out = [(1, H, 1, W),                                                       # the whole map
           (1, 1, 1, 1), (1, 1, W, W), (H, H, 1, 1), (H, H, W, W),             # a single pixel at each corner
           (H, H, 1, W), (1, H, W, W)]                                         # the last row, the last column
    for n in (1, 2, 3):     # windows ending in the plane's last 1, 2, 3 elements: the last piece of the plane is pulled back
        if n <= W:
            out.append((H, H, W - n + 1, W))
            out.append((max(1, H - 2), H, W - n + 1, W))

    def place(h, w):
        if 1 <= h <= H and 1 <= w <= W:
            y, x = rng.randint(1, H - h + 2), rng.randint(1, W - w + 2)
            out.append((y, y + h - 1, x, x + w - 1))
    for h in (kh - 1, kh, kh + 1, 2 * kh + 1):      # window sides of k - 1, k, k + 1 and 2 k + 1 for each grid dimension k
        for w in (kw - 1, kw, kw + 1, 2 * kw + 1):
            place(h, w)
        place(h, min(W, 5))
    for w in (kw - 1, kw, kw + 1, 2 * kw + 1):
        place(min(H, 5), w)
    if kh >= 2:             # smaller than the grid in one dimension, larger in the other (as far as the map allows)
        place(min(H, kh // 2), min(W, 2 * kw + 2))
    if kw >= 2:
        place(min(H, 2 * kh + 2), min(W, kw // 2))
    out += random_windows(rng, H, W, 4).tolist()
    return check_windows(np.array(out, np.int32), H, W)


def random_windows(rng, H, W, n):
    ys = np.sort(rng.randint(1, H + 1, (n, 2)), axis=1)
    xs = np.sort(rng.randint(1, W + 1, (n, 2)), axis=1)
    return check_windows(np.concatenate([ys, xs], axis=1).astype(np.int32), H, W)


def overlap_windows(H, W, seed, n=300):
    """n heavily overlapping windows around the middle of the map"""
    rng = np.random.RandomState(seed)
    cy, cx = rng.uniform(0.46, 0.54, n) * H, rng.uniform(0.46, 0.54, n) * W
    hh, hw = rng.uniform(0.02, 0.1, n) * H + 0.3, rng.uniform(0.02, 0.1, n) * W + 0.3
    w = np.stack([np.floor(cy - hh) + 1, np.floor(cy + hh) + 1, np.floor(cx - hw) + 1, np.floor(cx + hw) + 1], 1)
    w[:, :2] = np.clip(w[:, :2], 1, H)
    w[:, 2:] = np.clip(w[:, 2:], 1, W)
    return check_windows(w.astype(np.int32), H, W)


def windows_of(rows, H, W, kh, kw, seed):
    if rows == "edges":
        return edge_windows(H, W, kh, kw, seed)
    if rows == "overlap":
        return overlap_windows(H, W, seed)
    n = int(rows)           # the edge windows first, random ones up to n rows
    edges = edge_windows(H, W, kh, kw, seed)
    assert n > len(edges)
    return np.concatenate([edges, random_windows(np.random.RandomState(seed + 1), H, W, n - len(edges))])


# ---- maps --------------------------------------------------------------------------------------------------------------
KINDS = ("randn", "ties", "constant", "ramp_up", "ramp_down")
TIE_VALUES = np.array([-1.0, 0.0, 1.0, 2.0], np.float32)


def make_map(kind, C, H, W, rng):
    """float32 (C, H, W).  "ties": drawn from four values, so that most cells hold their maximum more than once; "constant": one
    value per plane (every element of a cell is its maximum: the first wins); the ramps rise / fall by 1 along the flat index of a
    plane (the last / first element of a cell wins), 3 c added on plane c.  All values are small integers or halves: exact."""
    if kind == "randn":
        return rng.randn(C, H, W).astype(np.float32)
    if kind == "ties":
        return TIE_VALUES[rng.randint(0, 4, (C, H, W))]
    c = np.arange(C, dtype=np.float32)[:, None, None]
    if kind == "constant":
        return np.ascontiguousarray(np.broadcast_to(1.5 + c, (C, H, W)), dtype=np.float32)
    flat = np.arange(H * W, dtype=np.float32).reshape(1, H, W)
    assert kind in ("ramp_up", "ramp_down"), kind
    return (flat if kind == "ramp_up" else -flat) + 3.0 * c


def closed_form_idx(kind, wins, C, W, kh, kw):
    """the winners of "constant" / "ramp_down" (the first element of every cell) and of "ramp_up" (the last), written down from the
    cell bounds alone: idx = (r0 + ys) W + c0 + xs, or (r0 + ye - 1) W + c0 + xe - 1"""
    last = {"constant": False, "ramp_down": False, "ramp_up": True}[kind]
    idx = np.zeros((len(wins), C, kh, kw), np.int32)
    for r, (rlo, rhi, clo, chi) in enumerate(np.asarray(wins).tolist()):
        for i, (ys, ye) in enumerate(cell_bounds(rhi - rlo + 1, kh)):
            for j, (xs, xe) in enumerate(cell_bounds(chi - clo + 1, kw)):
                y, x = (ye - 1, xe - 1) if last else (ys, xs)
                idx[r, :, i, j] = (rlo - 1 + y) * W + clo - 1 + x
    return idx.reshape(len(wins), C * kh * kw)


def tied_share(fmap, wins, kh, kw):
    """-> (cells of four or more elements whose maximum occurs more than once, cells of four or more elements), over all planes"""
    C = fmap.shape[0]
    tied = total = 0
    for rlo, rhi, clo, chi in np.asarray(wins).tolist():
        for ys, ye in cell_bounds(rhi - rlo + 1, kh):
            for xs, xe in cell_bounds(chi - clo + 1, kw):
                if (ye - ys) * (xe - xs) < 4:
                    continue
                cell = fmap[:, rlo - 1 + ys:rlo - 1 + ye, clo - 1 + xs:clo - 1 + xe].reshape(C, -1)
                tied += int(((cell == cell.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
                total += C
    return tied, total


# ---- the tables --------------------------------------------------------------------------------------------------------
SHAPES = [(5, 3, 5),
          (3, 1, 1), (2, 1, 3), (3, 2, 2),            # H W < 4 (the cells kernel's scalar branch) and H W == 4
          (8, 29, 50),
          (2, 128, 128), (2, 127, 130),               # either side of 16384 elements: a plane of 64 KB of fp32
          (2, 64, 128), (2, 91, 91),                  # either side of 8192 elements: a plane of 64 KB of 64-bit fixed point
          (257, 3, 5)]
GRIDS = [(6, 6), (7, 7), (1, 1), (2, 3), (3, 2), (3, 5),
         (16, 16),                                    # 256 cells: one group, no idle thread
         (15, 17),                                    # 255 cells: one group, one idle thread
         (17, 16), (1, 300)]                          # more than 256 cells: the generic kernel
MAIN = (8, 29, 50)

# (shape, grid, map kind, rows): rows is "edges", "overlap" or a row count
CASES = (
    # every grid on ties
    [(MAIN, g, "ties", "edges") for g in GRIDS] +
    [(MAIN, (6, 6), "randn", "edges"), (MAIN, (7, 7), "constant", "edges"), (MAIN, (2, 3), "ramp_up", "edges"),
     (MAIN, (3, 2), "ramp_down", "edges"), (MAIN, (3, 5), "randn", "edges"), (MAIN, (17, 16), "randn", "edges"),
     (MAIN, (15, 17), "ramp_up", "edges"), (MAIN, (1, 300), "ramp_down", "edges"),
     (MAIN, (6, 6), "ties", "overlap"), (MAIN, (3, 5), "randn", "overlap"),
     ((5, 3, 5), (6, 6), "randn", "edges"), ((5, 3, 5), (2, 3), "ties", "edges"), ((5, 3, 5), (1, 1), "constant", "edges"),
     ((5, 3, 5), (3, 5), "ramp_up", "edges"), ((5, 3, 5), (3, 2), "ramp_down", "edges"),
     ((3, 1, 1), (6, 6), "randn", "edges"), ((3, 1, 1), (1, 1), "constant", "edges"), ((3, 1, 1), (17, 16), "randn", "edges"),
     ((2, 1, 3), (2, 3), "ties", "edges"), ((2, 1, 3), (7, 7), "ramp_down", "edges"), ((2, 1, 3), (3, 2), "ramp_up", "edges"),
     ((3, 2, 2), (3, 2), "ties", "edges"), ((3, 2, 2), (6, 6), "ramp_up", "edges"), ((3, 2, 2), (1, 1), "randn", "edges"),
     ((2, 128, 128), (6, 6), "ties", "edges"), ((2, 128, 128), (3, 5), "randn", "edges"), ((2, 128, 128), (7, 7), "ties", "overlap"),
     ((2, 127, 130), (7, 7), "ties", "edges"), ((2, 127, 130), (2, 3), "randn", "edges"), ((2, 127, 130), (1, 300), "ramp_up", "edges"),
     ((2, 127, 130), (6, 6), "randn", "overlap"),
     ((2, 64, 128), (6, 6), "randn", "edges"), ((2, 64, 128), (3, 2), "ties", "edges"), ((2, 64, 128), (2, 3), "ties", "overlap"),
     ((2, 91, 91), (7, 7), "ties", "edges"), ((2, 91, 91), (3, 5), "randn", "edges"), ((2, 91, 91), (6, 6), "ties", "overlap"),
     ((257, 3, 5), (6, 6), "randn", "edges"), ((257, 3, 5), (16, 16), "ties", "edges"), ((257, 3, 5), (15, 17), "randn", "edges"),
     ((257, 3, 5), (2, 3), "ties", "edges"),
     # the two row counts: 600 rows of 64 channels at 7 x 7 (5 channels a block, 7 slices: a thread walks two channels), 4097 rows
     # (more rows than the 4096 blocks the slices are sized for: one slice)
     ((64, 29, 50), (7, 7), "ties", 600), ((3, 29, 50), (6, 6), "ties", 4097)])


def case_id(case):
    (C, H, W), (kh, kw), kind, rows = case
    return "%dx%dx%d-%dx%d-%s-%s" % (C, H, W, kh, kw, kind, rows)


def seed_of(case):
    (C, H, W), (kh, kw), kind, rows = case
    return (C * 7919 + H * 131 + W * 17 + kh * 1009 + kw * 37 + KINDS.index(kind) * 5 + len(str(rows))) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def windows_of_case(case):
    (C, H, W), (kh, kw), kind, rows = case
    wins = windows_of(rows, H, W, kh, kw, seed_of(case))
    wins.setflags(write=False)
    return wins


def labels_of_case(case):
    (C, H, W), (kh, kw), kind, rows = case
    R = len(windows_of_case(case))
    return plan(C, H, W, R, kh, kw, False) | plan(C, H, W, R, kh, kw, True)


def labels_of_tables(cases=None):
    labels = set()
    for case in (CASES if cases is None else cases):
        labels |= labels_of_case(case)
    return labels


@functools.lru_cache(maxsize=None)
def inputs(case):
    """the inputs and the reference of one case, computed once and shared by the tests (read-only).  The backward pass takes the
    REFERENCE's idx, with every seventh row set to -1 throughout (a row whose cells found no winner), a fiftieth of the other
    entries too, and a tenth of gout exactly zero; gmap0 is a non-zero map."""
    (C, H, W), (kh, kw), kind, rows = case
    rng = np.random.RandomState(seed_of(case))
    wins = windows_of_case(case)
    R, D = len(wins), C * kh * kw
    fmap = make_map(kind, C, H, W, rng)
    out, idx = forward(fmap, wins, kh, kw)
    bidx = idx.copy()
    bidx[3::7] = -1
    bidx[rng.rand(R, D) < 0.02] = -1
    gout = rng.randn(R, D).astype(np.float32)
    gout[rng.rand(R, D) < 0.1] = 0.0
    gout[0, 0] = 0.0
    assert np.any(np.all(bidx < 0, axis=1)) and np.any((gout == 0.0) & (bidx >= 0))
    gmap0 = rng.randn(C, H, W).astype(np.float32)
    gmap0[np.abs(gmap0) < 1e-3] = 1.0
    gmap, count, abs_sum = backward(gout, bidx, (C, H, W), gmap0)
    c = dict(C=C, H=H, W=W, kh=kh, kw=kw, kind=kind, R=R, D=D, wins=wins, fmap=fmap, out=out, idx=idx, bidx=bidx, gout=gout,
             gmap0=gmap0, gmap=gmap, count=count, abs_sum=abs_sum)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
