"""The case tables of tests/test_gpu_compact_ops.py and a numpy restatement of what the launches of a channel-compact
dropout block gather and scatter (include/frcnn_hip_compact.h; csrc/net.cpp plan_compact / pack_compact / wgrad_args,
csrc/convx.hip pack_x_job with PackXJob::oidx / cidx / Cs / bias_dst, csrc/conv.hip wgrad_reduce_map_kernel, the omap line of
csrc/wgradx.hip).

A block of width C whose SpatialDropout keeps nk filters runs six launches on the kept channels.  cin is the width of the
block's input, nb the number of filters of its second convolution (the model has nb = C; the op tests also take the
neighbouring width 64, the smallest conv_wgradx takes), idx[C] the step's table: the kept filters in ascending order, then -1.
    role     launch                                                     table          tensors
    fwd0     forward of (b, 0):        K = cin,  M = nkM                oidx = idx     out compact [nkM]
    fwd1     forward of (b, 1):        K = nkK,  M = nb                 cidx = idx     in compact, nkK of its nkM rows read
    dgrad1   input gradient of (b, 1): K = nb,   M = nkM  (+ post)      cidx = idx     gin compact [nkM], stored
    dgrad0   input gradient of (b, 0): K = nkK,  M = cin, accumulating  oidx = idx     gout compact, nkK of its nkM rows read
    wgrad1   weight gradient of (b, 1): Cin = nkM, O = nb               cmap = idx     in compact
    wgrad0   weight gradient of (b, 0): Cin = cin, O = nkM              omap = idx     gout compact
nkM = min(C, ceil64(nk)) sizes a filter / tile dimension, nkK = min(C, ceil16(nk)) a K dimension (sizes(), as plan_compact).

As in tests/convx_plan.py the restatement only LABELS the GPU cases, so that tests/test_compact_plan.py can check that the tables
reach every label of REQUIRED; the launch plans and the error bound are convx_plan's (x3_plan, wgradx_plan, split_bound,
representation_bound), the block's eligibility width_plan.compact_plan's: nothing of them is restated here."""
import zlib

import numpy as np

import conv_plan as CP
import convx_plan as XP
import width_plan as WP
from width_plan import cdiv

PAD = 1
CIN = 64            # width of the block's input: the smallest conv_wgradx_eligible takes
ROLES = ("fwd0", "fwd1", "dgrad1", "dgrad0", "wgrad1", "wgrad0")
CONV_ROLES = ROLES[:4]
KINDS = ("first", "last", "random", "ends")
AMAX_FACTOR = 2.0 ** 10   # amax_in_dropped: a dropped filter carries weights this many times the kept ones


def sizes(C, nk):
    """net.cpp plan_compact -> (nkM, nkK)"""
    return min(C, cdiv(nk, 64) * 64), min(C, cdiv(nk, 16) * 16)


def kept_set(C, nk, kind, seed=0):
    """nk of C filters, ascending.  first / last: the first / last nk; random: a random set; ends: a random set that holds
    both filter 0 and filter C - 1 (nk >= 2)"""
    assert 1 <= nk < C and kind in KINDS
    if kind == "first":
        return list(range(nk))
    if kind == "last":
        return list(range(C - nk, C))
    rng = np.random.RandomState(zlib.crc32(repr((C, nk, kind, seed)).encode()) & 0x7FFFFFFF)
    if kind == "ends":
        assert nk >= 2
        return sorted([0, C - 1] + list(1 + rng.permutation(C - 2)[:nk - 2]))
    return sorted(rng.permutation(C)[:nk].tolist())


def table(C, kept):
    """the step's table (net.cpp plan_compact): the kept filters, then -1"""
    return np.array(list(kept) + [-1] * (C - len(kept)), np.int32)


# ---- the semantics, in numpy --------------------------------------------------------------------------------------------
def gather_weights(W, oidx, nO, cidx, nC):
    """Wg[o'][c'] = W[oidx[o']][cidx[c']], zeros where either entry is negative; a table of None is the identity"""
    W = np.asarray(W)
    o = np.arange(nO) if oidx is None else np.asarray(oidx[:nO])
    c = np.arange(nC) if cidx is None else np.asarray(cidx[:nC])
    out = np.zeros((nO, nC) + W.shape[2:], W.dtype)
    oo, cc = np.nonzero(o >= 0)[0], np.nonzero(c >= 0)[0]
    out[np.ix_(oo, cc)] = W[np.ix_(o[oo], c[cc])]
    return out


def gather_bias(b, oidx, nO):
    """bias_dst[o'] = b[oidx[o']], 0 for a negative entry"""
    o = np.arange(nO) if oidx is None else np.asarray(oidx[:nO])
    out = np.zeros(nO, np.asarray(b).dtype)
    out[o >= 0] = np.asarray(b)[o[o >= 0]]
    return out


def scatter_add(gw, part, omap, cmap):
    """gw[omap[o']][cmap[c']] += part[o'][c'] for the pairs with two non-negative entries (in gw's precision); -> gw"""
    O, Cn = part.shape[:2]
    o = np.arange(O) if omap is None else np.asarray(omap[:O])
    c = np.arange(Cn) if cmap is None else np.asarray(cmap[:Cn])
    oo, cc = np.nonzero(o >= 0)[0], np.nonzero(c >= 0)[0]
    gw[np.ix_(o[oo], c[cc])] += part[np.ix_(oo, cc)].astype(gw.dtype)
    return gw


def scatter_add_bias(gb, part, omap):
    o = np.arange(len(part)) if omap is None else np.asarray(omap[:len(part)])
    gb[o[o >= 0]] += np.asarray(part)[o >= 0].astype(gb.dtype)
    return gb


# ---- a launch ------------------------------------------------------------------------------------------------------------------
def launch(role, C, nk, nb, hw, cin=CIN):
    """-> dict: the sizes of role's launch of a block of width C with nk kept, input width cin, nb second-convolution filters, on
    the map hw = (H, W) at padding 1.  full = (O_full, C_full) of the weight tensor, gather = which table carries idx ("o" |
    "c"), n = (nO, nC) of the entry point, shape = the forward shape (K, H, W, M, 3, 1) whose conv_x3 launch it is (convx_plan)
    or the weight-gradient shape (Cin, H, W, O, 3, 1), rows = the rows the compact tensor of the launch has (its producer's
    nkM) where the launch reads fewer."""
    H, W = hw
    nkM, nkK = sizes(C, nk)
    d = dict(role=role, C=C, nk=nk, nb=nb, cin=cin, H=H, W=W, nkM=nkM, nkK=nkK)
    if role == "fwd0":
        d.update(full=(C, cin), gather="o", n=(nkM, cin), shape=(cin, H, W, nkM, 3, PAD), live=nk)
    elif role == "fwd1":
        d.update(full=(nb, C), gather="c", n=(nb, nkK), shape=(nkK, H, W, nb, 3, PAD), rows=nkM, live=nb)
    elif role == "dgrad1":
        d.update(full=(nb, C), gather="c", n=(nb, nkM), shape=(nb, H, W, nkM, 3, PAD), live=nk)
    elif role == "dgrad0":
        d.update(full=(C, cin), gather="o", n=(nkK, cin), shape=(nkK, H, W, cin, 3, PAD), rows=nkM, live=cin)
    elif role == "wgrad1":
        d.update(full=(nb, C), gather="c", n=(nb, nkM), shape=(nkM, H, W, nb, 3, PAD))
    elif role == "wgrad0":
        d.update(full=(C, cin), gather="o", n=(nkM, cin), shape=(cin, H, W, nkM, 3, PAD))
    else:
        raise KeyError(role)
    return d


def eligible(C, nk, nb, cin=CIN):
    """net.cpp plan_compact's shape conditions for a block that is not the first (its first convolution computes an input
    gradient), with nb in place of the block's own width as the second convolution's filter count"""
    nkM, nkK = sizes(C, nk)
    return (0 < nk and nkK < C and WP.conv_x3_eligible(cin, nkM, 3) and WP.conv_x3_eligible(nkK, nb, 3) and
            WP.conv_x3_eligible(nb, nkM, 3) and WP.conv_x3_eligible(nkK, cin, 3) and WP.conv_wgradx_eligible(nkM, nb, 3) and
            WP.conv_wgradx_eligible(cin, nkM, 3))


def labels(L, kind, amax=None, form=None, post=False):
    """labels of one launch (a dict of launch()): the role, the table's edges, the plan of the launch it becomes"""
    out = {L["role"], "kept_" + kind}
    nkM, nkK, nk, C = L["nkM"], L["nkK"], L["nk"], L["C"]
    n_tab = {"fwd0": nkM, "fwd1": nkK, "dgrad1": nkM, "dgrad0": nkK, "wgrad1": nkM, "wgrad0": nkM}[L["role"]]
    if n_tab > nk:
        out.add("pad_rows")
    if nkM == C:
        out.add("nkM_eq_C")
    if (nkK // XP.CX_CH) % 2 and L["role"] in ("fwd1", "dgrad0"):
        out.add("odd_chunks")
    if kind == "ends":
        out.add("first_and_last_kept")
    if amax and L["role"] in CONV_ROLES:   # (a weight gradient does not read the weights)
        out.add("amax_in_" + amax)
    if form is not None:
        out.add("form_" + XP_FORMS[form])
    if L["role"] in CONV_ROLES:
        p = XP.x3_plan(L["shape"], post=post)
        out.add("splitk" if p["splitK"] > 1 else "one_slab")
        out.add("bm%d" % p["bm"])
        if post:
            out.add("post")
            out.add("post_fold" if p["where"] == "fold" else "post_inline")
    else:
        p = XP.wgradx_plan(L["shape"])
        got = XP.wgradx_labels(p)
        out |= got & {"wg_uneven", "wg_one_tile", "wg_vec1", "wg_vec2", "wg_partial_tile"}
    return out


XP_FORMS = {0: "bf16x6", 1: "f16x3"}

# ---- the case tables ------------------------------------------------------------------------------------------------------------
MAPS = {"9x12": (9, 12), "12x16": (12, 16), "10x13": (10, 13)}   # the last: an odd width, conv_wgradx's unaligned loader
KEPT_COUNTS = {128: (1, 15, 16, 17, 63, 64, 65, 112), 192: (65, 176)}


def ccase(name, C, nk, kind, nb, hw, amax=None, roles=ROLES):
    return dict(name=name, C=C, nk=nk, kind=kind, nb=nb, hw=MAPS.get(hw, hw), amax=amax, roles=tuple(roles))


CASES = [
    # C = 128: every kept count around the multiples of 16 and 64; the four kinds of kept set in turn
    ccase("c128_k1", 128, 1, "first", 64, "9x12"),
    ccase("c128_k15", 128, 15, "random", 64, "12x16"),
    ccase("c128_k16", 128, 16, "last", 64, "9x12"),
    ccase("c128_k17", 128, 17, "ends", 64, "10x13"),
    ccase("c128_k63", 128, 63, "ends", 64, "12x16", amax="dropped"),
    ccase("c128_k64", 128, 64, "random", 64, "9x12", amax="kept"),
    ccase("c128_k65", 128, 65, "random", 128, "12x16", amax="dropped"),        # the block of the contract test: nb = C
    ccase("c128_k65_last", 128, 65, "last", 64, "10x13", amax="kept"),
    ccase("c128_k112", 128, 112, "ends", 64, "9x12"),                         # nkM == C while nkK < C
    ccase("c128_k112_first", 128, 112, "first", 128, "10x13", amax="kept"),
    # C = 192: nk = 65 -> nkM = 128, nkK = 80 (five chunks); nk = 176 -> nkM = 192 = C, nkK = 176 (eleven chunks: split K)
    ccase("c192_k65", 192, 65, "ends", 64, "12x16", amax="dropped"),
    ccase("c192_k65_last", 192, 65, "last", 128, "9x12"),
    ccase("c192_k176", 192, 176, "random", 64, "12x16", amax="kept"),
    ccase("c192_k176_first", 192, 176, "first", 128, "9x12"),
    # the weight gradient's launch plans: one pixel tile; more tiles than splits (192 x 192: 9 tile pairs -> 28 splits of 30 tiles)
    ccase("wg_one_tile", 128, 65, "random", 64, (4, 16), roles=("wgrad1", "wgrad0")),
    ccase("wg_one_tile_first", 128, 17, "last", 64, (4, 16), roles=("wgrad1", "wgrad0")),
    ccase("wg_uneven", 192, 176, "ends", 192, (20, 96), roles=("wgrad1",)),
    ccase("wg_uneven_o", 192, 176, "random", 192, (8, 240), roles=("wgrad0",)),
]
# the wg_uneven cases take the block's input as wide as the block (cin = C), which makes 9 tile pairs of the first convolution too
WIDE_CIN = {"wg_uneven": 192, "wg_uneven_o": 192}


def find(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def runs():
    """every launch of tests/test_gpu_compact_ops.py's op tests: dicts of case, role, post (dgrad1 runs with and without the
    fused activation backward); each runs in both operand forms"""
    out = []
    for c in CASES:
        for role in c["roles"]:
            for post in ((False, True) if role == "dgrad1" else (False,)):
                out.append(dict(name=c["name"], role=role, post=post))
    return out


def launch_of_run(r):
    c = find(r["name"])
    return launch(r["role"], c["C"], c["nk"], c["nb"], c["hw"], WIDE_CIN.get(c["name"], CIN))


def labels_of_run(r, form=None):
    c = find(r["name"])
    return labels(launch_of_run(r), c["kind"], c["amax"], form, r["post"])


def run_id(r):
    return "%s-%s%s" % (r["role"], r["name"], "-post" if r["post"] else "")


REQUIRED = set(ROLES) | {
    "pad_rows", "nkM_eq_C", "odd_chunks", "first_and_last_kept", "amax_in_dropped", "amax_in_kept", "form_bf16x6", "form_f16x3",
    "splitk", "one_slab", "wg_uneven", "wg_one_tile", "wg_vec2", "post", "kept_first", "kept_last", "kept_random", "kept_ends",
}
# every (role, label) pair the tables must reach as well: an edge of the table counts per launch that reads the table
REQUIRED_PAIRS = {(role, l) for role in ROLES for l in ("pad_rows", "nkM_eq_C", "first_and_last_kept", "kept_first", "kept_last",
                                                        "kept_random")}
REQUIRED_PAIRS |= {(role, l) for role in CONV_ROLES for l in ("amax_in_dropped", "amax_in_kept")}
REQUIRED_PAIRS |= {("fwd1", "odd_chunks"), ("dgrad0", "odd_chunks"), ("fwd1", "splitk"), ("dgrad0", "splitk"), ("dgrad1", "splitk"),
                   ("fwd0", "one_slab"), ("dgrad1", "post_inline"), ("dgrad1", "post_fold"), ("wgrad1", "wg_uneven"),
                   ("wgrad0", "wg_uneven"), ("wgrad1", "wg_one_tile"), ("wgrad0", "wg_one_tile"), ("wgrad1", "wg_vec2"),
                   ("wgrad0", "wg_vec2")}


def reached(rs):
    """-> (labels, (role, label) pairs) the runs reach, both operand forms"""
    L, P = set(), set()
    for r in rs:
        for form in XP_FORMS:
            got = labels_of_run(r, form)
            L |= got
            P |= {(r["role"], l) for l in got}
    return L, P


def short(rs):
    """what of REQUIRED / REQUIRED_PAIRS the runs do not reach"""
    L, P = reached(rs)
    return sorted(REQUIRED - L), sorted(REQUIRED_PAIRS - P)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rng_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def weights(rng, full, kept, gather, amax=None):
    """the FULL weight tensor [O_full][C_full][3][3] and bias.  amax = "dropped": every weight of one dropped filter / channel
    is AMAX_FACTOR times a kept-sized one (the tensor's largest magnitude lies there, ten binades above the kept part's);
    "kept": the largest magnitude of the tensor is planted in the first kept filter / channel."""
    O, Cc = full
    w = (rng.randn(O, Cc, 3, 3) / np.sqrt(Cc * 9)).astype(np.float32)
    b = rng.randn(O).astype(np.float32)
    n = O if gather == "o" else Cc
    dropped = sorted(set(range(n)) - set(kept))
    if amax == "dropped":
        d = dropped[len(dropped) // 2]
        if gather == "o":
            w[d] *= np.float32(AMAX_FACTOR)
        else:
            w[:, d] *= np.float32(AMAX_FACTOR)
    elif amax == "kept":
        top = np.float32(1.5 * np.abs(w).max())
        if gather == "o":
            w[kept[0], 0, 1, 1] = top
        else:
            w[0, kept[0], 1, 1] = -top
    return w, b


def amax_lies_in_kept(w, kept, gather):
    part = w[kept] if gather == "o" else w[:, kept]
    return float(np.abs(part).max()) == float(np.abs(w).max())


SLOPE = np.float32(0.25)


def conv_inputs(r, rep=0):
    """the operands of one convolution run (roles fwd0, fwd1, dgrad1, dgrad0), repetition rep: the full weight tensor w / bias b,
    the tables, the host-gathered wg / bg, the tensor x the launch reads (K channels), the fp64 reference `want` of the dense
    operation on the gathered operands and the same on magnitudes `mag`, op = the bilinear operation (for the bounds).  The
    activation backward of a post run is left to the caller (it needs the convolution's own bound)."""
    c, L = find(r["name"]), launch_of_run(r)
    rng = rng_of("compact", r["name"], r["role"], bool(r["post"]), rep)
    kept = kept_set(c["C"], c["nk"], c["kind"])
    idx = table(c["C"], kept)
    w, b = weights(rng, L["full"], kept, L["gather"], c["amax"])
    nO, nC = L["n"]
    oidx, cidx = (idx, None) if L["gather"] == "o" else (None, idx)
    wg = gather_weights(w, oidx, nO, cidx, nC)
    K, H, W, M = L["shape"][:4]
    x = rng.randn(K, H, W).astype(np.float32)
    d = dict(case=c, L=L, kept=kept, idx=idx, oidx=oidx, cidx=cidx, w=w, b=b, wg=wg, x=x, K=K, M=M, H=H, W=W, nO=nO, nC=nC,
             slope=None, bg=None, rng=rng)
    if r["role"] in ("fwd0", "fwd1"):
        d["bg"] = gather_bias(b, oidx, nO)
        d["slope"] = SLOPE if r["role"] == "fwd1" else None      # (b, 1) reads (b, 0)'s pre-activations through their PReLU
        d["act"] = CP.activate(x, d["slope"], None)
        d["op"] = lambda a, ww: CP.ref_forward(a, ww, None, PAD)
        d["want"] = CP.ref_forward(d["act"], wg, d["bg"], PAD)
        d["mag"] = CP.ref_forward(np.abs(d["act"]), np.abs(wg), np.abs(d["bg"]), PAD)
    else:
        d["act"] = x
        d["op"] = lambda a, ww: CP.ref_input_gradient(a, ww, PAD, H, W)
        d["want"] = d["op"](x, wg)
        d["mag"] = d["op"](np.abs(x), np.abs(wg))
    return d


def live_rows(d):
    """rows of the launch's output that a non-negative table entry names (all of them where the table gathers channels of K)"""
    role = d["L"]["role"]
    if role == "fwd0":
        return np.asarray(d["oidx"][:d["M"]]) >= 0
    if role == "dgrad1":
        return np.asarray(d["cidx"][:d["M"]]) >= 0
    return np.ones(d["M"], bool)
