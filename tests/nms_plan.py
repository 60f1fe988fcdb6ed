"""NMS problems with closed-form answers (tests/test_gpu_nms_scan.py) and a plain restatement of which wave of the greedy
scan (csrc/nms.hip nms_reduce_body) carries each "kept row p suppresses q" bit.

The restatement only LABELS the problems with the roles they reach, so that tests/test_nms_plan.py can check that the tables
still reach every one of them: it is no evidence that a role computes the right thing.  The GPU tests against the closed
forms and the oracle are.

A problem is described in SORTED POSITIONS 0 .. n-1, the order the scan walks (descending key = max-y):
  position i     y1 = 0, y2 = 4n - i; a slot of its own, x1 = 64 i, x2 = x1 + 32: boxes in different slots never overlap
  pair (p, q)    p < q: q takes p's slot.  IoU = (4n - q + 1) / (4n - p + 1) >= 0.75: p suppresses q at THR = 0.4 and nothing else
                 happens.  A suppressor may have many victims; a victim is never a suppressor
  chain (s, m)   positions s .. s + m - 1: x1 = 64 s + 30 j, x2 = x1 + 100.  Neighbours have IoU ~ 0.54, next-but-one members
                 ~ 0.26: exactly the even members survive, and each decision waits for the one before it
Rows are then permuted (seeded), so the sorted order is not the row order.  Every coordinate and area is an integer below
2^24: fp32 is exact and no IoU sits near the threshold.  The expected pick list is closed form: the 1-based rows of the
non-victim positions, in position order."""
import numpy as np

# ---- the constants of csrc/nms.hip (tests/test_nms_plan.py compares them with the file's #defines) ----------------------
LEAD = 4                               # NMS_LEAD
NU = LEAD                              # NMS_NU: helper waves, words g + 2 .. g + 1 + NU
BG_ITEMS = 4                           # NMS_BG_ITEMS: 64-word pieces a background wave holds in registers per step
RED_THREADS = 1024                     # NMS_RED_THREADS
BG_WAVES = RED_THREADS // 64 - 2 - NU  # NMS_BG_WAVES = 10
RANK_SLICE = 256                       # NMS_RANK_SLICE
THR = 0.4


def cdiv(a, b):
    return -(-a // b)


# ---- the generator --------------------------------------------------------------------------------------------------
def make(name, n, pairs=(), chains=(), seed=1, equal_keys=False):
    """-> dict(name, n, thr, rows [n][4] fp32 in ROW order, expect = the closed-form pick list (1-based rows), row_of [position]
    -> 0-based row, pairs, chains, victims = the suppressed positions)."""
    pairs = [(int(p), int(q)) for p, q in pairs]
    pos = np.zeros((n, 4), np.float64)
    i = np.arange(n)
    pos[:, 0] = 64 * i
    pos[:, 3] = 4 * n if equal_keys else 4 * n - i
    victims = set()
    in_chain = set()
    for s, m in chains:
        assert 0 <= s and s + m <= n and not equal_keys
        # the slots the chain covers belong to its own positions
        assert 64 * s + 30 * (m - 1) + 100 < 64 * (s + m)
        for j in range(m):
            pos[s + j, 0] = 64 * s + 30 * j
            assert s + j not in in_chain
            in_chain.add(s + j)
            if j % 2:
                victims.add(s + j)
    pos[:, 2] = pos[:, 0] + 32
    for p in in_chain:
        pos[p, 2] = pos[p, 0] + 100
    sup = {p for p, q in pairs}
    for p, q in pairs:
        assert 0 <= p < q < n, (p, q)
        assert q not in sup and q not in victims and p not in in_chain and q not in in_chain, (p, q)
        pos[q, 0], pos[q, 2] = pos[p, 0], pos[p, 2]
        victims.add(q)
    assert pos.max() < 2 ** 24 and (pos[:, 2] - pos[:, 0] + 1).max() * (4 * n + 1) < 2 ** 24
    if equal_keys:
        row_of = np.arange(n)[::-1].copy()     # equal keys: the higher row goes first, whatever the seed
    else:
        row_of = np.random.RandomState(seed).permutation(n)
    rows = np.zeros((n, 4), np.float32)
    rows[row_of] = pos
    expect = [int(row_of[p]) + 1 for p in range(n) if p not in victims]
    return dict(name=name, n=n, thr=THR, rows=rows, expect=expect, row_of=row_of, pairs=pairs, chains=list(chains),
                victims=sorted(victims))


def with_classes(prob):
    """Classes (int32, one per ROW) under which every second pair has suppressor and victim in different classes, and the
    closed form: non-victims plus cross-class victims, in position order.  A suppressor's cross-class victims all differ in
    class (they share its slot and would suppress each other); a chain stays in one class."""
    n = prob["n"]
    cls_pos = 1 + np.arange(n) % 3
    for s, m in prob["chains"]:
        cls_pos[s:s + m] = 2
    victims = set(prob["victims"])
    crossed = {}
    for k, (p, q) in enumerate(prob["pairs"]):
        if k % 2:
            crossed[p] = crossed.get(p, 0) + 1
            cls_pos[q] = cls_pos[p] + 3 * crossed[p]     # 4 .. : never a class of p, nor of another crossed victim of p
            victims.discard(q)
        else:
            cls_pos[q] = cls_pos[p]
    cls = np.zeros(n, np.int32)
    cls[prob["row_of"]] = cls_pos
    expect = [int(prob["row_of"][p]) + 1 for p in range(n) if p not in victims]
    return cls, expect


# ---- the tables of tests/test_gpu_nms_scan.py -----------------------------------------------------------------------
SCAN_N = 72 * 64 - 5            # nw = 72: behind group 0 (words 6 .. 71) a second 64-word piece of two words, 70 and the last
SCAN_GROUPS = (0, 12)           # suppressor groups: two pieces behind group 0, one behind group 12
SCAN_RANKS = (0, 9, 10, 19, 20, 39, 40, 62)
SCAN_DISTANCES = (1, 2, 3, 4, 5, 6, 7, 69, 70)   # word distances suppressor -> victim; 0 and the last word apart
SCAN_CHAIN = (64 * 30 + 50, 150)                 # crosses two group boundaries, fills groups 31 and 32


def _scan_pairs():
    """Suppressors at offsets = ranks 0, 9, .. 62 of groups 0 and 12 (every position before them in the group is kept, so a
    suppressor's offset is its rank); one victim per (suppressor, word distance) wherever that word exists, one in the last
    word, and the single in-group position that disturbs no rank (offset 63) as the distance-0 victim of rank 0 (group 0) and
    of rank 62 (group 12).  The very last position is a victim."""
    nw = cdiv(SCAN_N, 64)
    pairs = []
    for gi, G in enumerate(SCAN_GROUPS):
        for k, r in enumerate(SCAN_RANKS):
            p = 64 * G + r
            off = 2 + 7 * k + 3 * gi                    # 2 .. 51 from group 0, 5 .. 54 from group 12: all distinct per word
            for d in SCAN_DISTANCES:
                if G + d < nw - 1:
                    pairs.append((p, 64 * (G + d) + off))
            last = SCAN_N - 1 if (gi, k) == (1, 7) else 64 * (nw - 1) + off
            pairs.append((p, last))
        pairs.append((64 * G + (0 if gi == 0 else 62), 64 * G + 63))
    return pairs


def _edge(n):
    """(0, n - 1), plus one pair inside the last group -- the last FULL group where the last one holds fewer than three boxes"""
    g0 = 64 * ((n - 1) // 64)
    if n - g0 >= 3:
        second = (max(g0, 1), n - 2)
    else:
        second = (g0 - 63, g0 - 1)
    return make("edge_%d" % n, n, pairs=[(0, n - 1), second], seed=n)


SCAN_CASE = make("scan", SCAN_N, pairs=_scan_pairs(), chains=[SCAN_CHAIN], seed=72)
EDGE_SIZES = [_edge(64 * k + e) for k in range(1, 8) for e in (-1, 0, 1)]
ALL_KEPT = make("all_kept", 1000, seed=2)
ONE_KEPT = make("one_kept", 1000, pairs=[(0, q) for q in range(1, 1000)], seed=3)
CHAIN_ALONE = make("chain_alone", SCAN_CHAIN[1], chains=[(0, SCAN_CHAIN[1])], seed=4)
# one key for all 700 rows: sorted position i is row 700 - i (1-based), the tie rule runs across three blocks of RANK_SLICE keys.
# Two identical pairs; of each the partner with the lower row loses: rows 6 (partner 650, two blocks away) and 300 (partner
# 301, the same block)
EQUAL_KEYS = make("equal_keys", 700, pairs=[(700 - 650, 700 - 6), (700 - 301, 700 - 300)], equal_keys=True)
DEGENERATE = dict(name="degenerate", n=5, thr=0.5, expect=[4, 3],   # 0 / 0 = NaN: `IoU <= t` is false, the box goes
                  rows=np.array([[10, 10, 9, 30], [10, 10, 9, 31], [10, 10, 9, 32], [100, 5, 120, 33], [10, 12, 9, 29.5]],
                                np.float32))

CLOSED_FORM = [SCAN_CASE] + EDGE_SIZES + [ALL_KEPT, ONE_KEPT, CHAIN_ALONE, EQUAL_KEYS]
ALL = CLOSED_FORM + [DEGENERATE]


# ---- the greedy pass restated in fp32, and the labels ----------------------------------------------------------------
def sort_order(key):
    """positions -> rows: descending key, ties to the higher row (nms.hip: ascending key, ties ascending row, picks from the end)"""
    n = len(key)
    return np.lexsort((-np.arange(n), -np.asarray(key, np.float64)))


def _suppresses(b, area, p, lo, hi, thr):
    """S[p][lo:hi] of sorted boxes b: the fp32 arithmetic of nms.lua:78-96, every operation rounded on its own"""
    one = np.float32(1)
    xx1 = np.maximum(b[lo:hi, 0], b[p, 0]); yy1 = np.maximum(b[lo:hi, 1], b[p, 1])
    xx2 = np.minimum(b[lo:hi, 2], b[p, 2]); yy2 = np.minimum(b[lo:hi, 3], b[p, 3])
    w = np.maximum(np.float32(0), (xx2 - xx1) + one)
    h = np.maximum(np.float32(0), (yy2 - yy1) + one)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / ((area[lo:hi] + area[p]) - inter)
        return ~(iou <= np.float32(thr))


LABELS = ("diag", "next_word") + tuple("helper%d" % k for k in range(1, NU + 1)) + \
    ("bg_reg_chunk0", "bg_reg_chunk1", "bg_now_chunk0", "bg_now_chunk1")


def role(p, r, q, nw):
    """The role that carries "the kept row at position p, rank r among the kept rows of its group, suppresses position q"."""
    G = p // 64
    d = q // 64 - G
    if d == 0:
        return "diag"
    if d == 1:
        return "next_word"
    if d <= 1 + NU:
        return "helper%d" % (d - 1)
    wfirst = G + 2 + NU
    nchunks = cdiv(nw - wfirst, 64)
    c = (q // 64 - wfirst) // 64
    seq = (r // BG_WAVES) * nchunks + c        # a wave takes the rows r = wave, wave + BG_WAVES, ..; piece by piece
    return "%s_chunk%d" % ("bg_reg" if seq < BG_ITEMS else "bg_now", min(c, 1))


def analyse(rows, thr, key=None, drop=()):
    """The greedy pass over `rows` (key: the sort keys, default max-y) -> dict(pick = the 1-based pick list, kept_max = most
    kept rows of a 64-group, rounds_max = most ballot rounds the diagonal loop of a group takes, sole = {label: number of
    suppressed boxes ALL of whose kept suppressors act through that one role}).  drop: roles behind the diagonal whose ORs
    are left out -- the pick list a scan with that role broken would give."""
    assert "diag" not in drop
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    nw = cdiv(n, 64)
    order = sort_order(rows[:, 3] if key is None else key)
    b = rows[order, :4]
    area = ((b[:, 2] - b[:, 0]) + np.float32(1)) * ((b[:, 3] - b[:, 1]) + np.float32(1))
    removed = np.zeros(n, bool)
    labs = np.zeros(n, np.int64)                # bit l: a kept suppressor acts on this position through LABELS[l]
    kept = np.zeros(n, bool)
    kept_max = rounds_max = 0
    for g in range(nw):
        lo, hi = 64 * g, min(64 * g + 64, n)
        m = hi - lo
        # the diagonal block, all rows: D[u][t] = the box at lo + u suppresses the box at lo + t (u < t)
        D = np.zeros((m, m), bool)
        for u in range(m - 1):
            D[u, u + 1:] = _suppresses(b, area, lo + u, lo + u + 1, hi, thr)
        # the ballot rounds of wave 0: a box is decided once every box of its column is; kept if no kept box suppresses it
        done = removed[lo:hi].copy()
        kg = np.zeros(m, bool)
        rounds = 0
        while not done.all():
            ready = ~done & ~(D & ~done[:, None]).any(0)
            kg |= ready & ~(D & kg[:, None]).any(0)
            done |= ready
            rounds += 1
        rounds_max = max(rounds_max, rounds)
        kept[lo:hi] = kg
        kept_max = max(kept_max, int(kg.sum()))
        for r, u in enumerate(np.nonzero(kg)[0]):
            p = lo + int(u)
            if p + 1 >= n:
                continue
            hit = np.nonzero(_suppresses(b, area, p, p + 1, n, thr))[0] + p + 1
            for w in np.unique(hit // 64):
                lab = role(p, r, int(w) * 64, nw)
                if lab in drop:
                    continue
                removed[hit[hit // 64 == w]] = True
                labs[hit[hit // 64 == w]] |= 1 << LABELS.index(lab)
    assert not (kept & removed).any()
    sole = {}
    for l, name in enumerate(LABELS):
        c = int((removed & (labs == 1 << l)).sum())
        if c:
            sole[name] = c
    return dict(pick=[int(order[p]) + 1 for p in np.nonzero(kept)[0]], kept_max=kept_max, rounds_max=rounds_max, sole=sole)


def rank_blocks_of_equal_keys(key):
    """(blocks, shared): the most RANK_SLICE-key blocks of nms_rank_body that one key value's rows lie in, and whether two of
    them share a block (the tie rule on the diagonal as well as off it)"""
    key = np.asarray(key)
    values, counts = np.unique(key, return_counts=True)
    best = (0, False)
    for v in values[counts > 1]:
        blocks = (np.nonzero(key == v)[0] // RANK_SLICE).tolist()
        best = max(best, (len(set(blocks)), len(blocks) > len(set(blocks))))
    return best


def labels_of(prob):
    """The labels a table entry reaches, from its boxes alone"""
    a = analyse(prob["rows"], prob["thr"])
    labels = set(a["sole"])
    if a["rounds_max"] == 64:
        labels.add("chain_full_group")
    blocks, shared = rank_blocks_of_equal_keys(prob["rows"][:, 3])
    if blocks >= 3 and shared:
        labels.add("equal_keys_across_rank_blocks")
    return labels


REQUIRED = set(LABELS) | {"chain_full_group", "equal_keys_across_rank_blocks"}
