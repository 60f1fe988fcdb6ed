"""The case tables of tests/test_gpu_heads_chain.py, a plain restatement of which path each case takes through the anchor
nets' sparse training chain -- csrc/heads.hip (six kernels, heads_plan_splits, heads_add_job, heads_chain_*), csrc/gemm.hip
(gemm_f32_group / gemm_group_kernel) and the per-net position helpers of csrc/elem.hip -- and the fp64 references, whole and
stage by stage.  include/frcnn_hip_heads.h says what the entry points do.

As in tests/gemm_plan.py the restatement only LABELS the GPU cases with the branches they reach, so that
tests/test_heads_plan.py can check that the tables still reach every one of them; the GPU tests against the references are the
evidence that a branch computes the right thing.  tests/test_heads_plan.py also anchors the references themselves: against a
plain fp64 dense convolution net, forward and backward.

One anchor net: in[Cin][H][W] -> k x k valid convolution to n filters (w3[n][ckk], ckk = Cin k k, bias3) -> PReLU (one slope) ->
1 x 1 convolution to 18 planes (w1[18][n], bias1), read and trained at P positions pos = y Wo + x of the Ho x Wo output map."""
import zlib

import numpy as np

from conv_plan import case
from width_plan import cdiv, head_splits

HEAD_OUT = 18
GB = 64                  # gemm_group_kernel: 64 x 64 tiles
GBK = 32                 # ... and K runs in multiples of 32
GROUP_MAX = 4
HD_GRID_CAP = 4096       # heads.hip hd_grid: blocks of 256 along x, grid-stride behind the cap
SLAB_POSITIONS = 4096    # the model's slab: n x 4096 partial sums per net
U = 2.0 ** -24


def rng_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ---- the grouped product -------------------------------------------------------------------------------------------------------
# A job is (M, N, K, orient, splits, add, pad): orient two letters -- A "k" (k-contiguous: sAm = K, sAk = 1) or "m" (sAm = 1,
# sAk = M); B "k" (sBk = 1, sBn = K) or "n" (sBk = N, sBn = 1); pad = ldc - N.
def gjob(M, N, K, orient, splits=1, add=False, pad=0):
    assert orient in ("kk", "kn", "mk", "mn")
    return dict(M=M, N=N, K=K, orient=orient, splits=splits, add=add, pad=pad)


def strides(j):
    """-> sAm, sAk, sBk, sBn, ldc of a job whose operands are dense"""
    sAm, sAk = (j["K"], 1) if j["orient"][0] == "k" else (1, j["M"])
    sBk, sBn = (1, j["K"]) if j["orient"][1] == "k" else (j["N"], 1)
    return sAm, sAk, sBk, sBn, j["N"] + j["pad"]


def chain_products(n, ckk, P, splits=1):
    """the six products of the chain in their real orientations (heads.hip heads_chain_*), by name"""
    return dict(HX=gjob(n, P, ckk, "kk", splits), OUT=gjob(HEAD_OUT, P, n, "kn"), GH=gjob(n, P, HEAD_OUT, "mn"),
                DX=gjob(P, ckk, n, "mn"), gW1=gjob(HEAD_OUT, n, P, "kk", add=True), gW=gjob(n, ckk, P, "kn", add=True))


def k_runs(K, splits):
    """gemm_f32_group: -> (kPer, the run lengths); a run may not be empty"""
    kper = cdiv(cdiv(K, max(1, splits)), GBK) * GBK
    ns = cdiv(K, kper)
    return kper, [min(kper, K - s * kper) for s in range(ns)]


def group_flags(jobs):
    """the kernel instantiation a group launches: job 0's unit strides, blocks or not"""
    sAm, sAk, sBk, sBn, _ = strides(jobs[0])
    return ("k" if sAk == 1 else "m") + ("k" if sBk == 1 else "n")


def job_flags(j):
    sAm, sAk, sBk, sBn, _ = strides(j)
    return ("k" if sAk == 1 else "m") + ("k" if sBk == 1 else "n")


GEMM_M_N = (1, 18, 63, 64, 65, 129)
GEMM_K = (1, 31, 32, 33, 72)


def group_labels(c):
    jobs = c["jobs"]
    L = {"kernel_" + group_flags(jobs), "jobs_%d" % len(jobs)}
    if c.get("role"):
        L.add("role_" + c["role"])
    live = [i for i, j in enumerate(jobs) if j["M"] > 0 and j["N"] > 0]
    for i, j in enumerate(jobs):
        if i not in live:
            L.add("zero_first" if i == 0 else "zero_last" if i == len(jobs) - 1 else "zero_middle")
            if live and min(live) < i < max(live):
                L.add("zero_between_live")
            continue
        for v in GEMM_M_N:
            if j["M"] == v:
                L.add("m_%d" % v)
            if j["N"] == v:
                L.add("n_%d" % v)
        if j["K"] in GEMM_K:
            L.add("k_%d" % j["K"])
        kper, runs = k_runs(j["K"], j["splits"])
        assert len(runs) == max(1, j["splits"]), (c["name"], i)
        if j["splits"] > 1:
            L.add("splits_%d" % j["splits"])
            if runs[-1] < kper:
                L.add("last_split_short")
            if j["splits"] == 3 and runs[-1] < kper:
                L.add("splits_3_short_last")
        else:
            L.add("splits_1")
            L.add("ep_add" if j["add"] else "ep_store")
            if j["pad"]:
                L.add("ldc_gt_n")
        if j["M"] % GB:
            L.add("m_tail")
        if j["N"] % GB:
            L.add("n_tail")
        if j["K"] % GBK:
            L.add("k_tail")
    # a unit stride that is an accident of a dimension of 1: the flags of the launch are not the job's natural ones
    nat0, f = jobs[0]["orient"], group_flags(jobs)
    if f != nat0 and any(j["orient"] == nat0 and job_flags(j) == nat0 for j in jobs[1:]):
        L.add("job0_accidental_flags")          # job 0 has N = 1 (P = 1), the later jobs run under flags that are not theirs
    if f == nat0 and any(job_flags(j) != f and j["M"] > 0 and j["N"] > 0 for j in jobs[1:]):
        L.add("later_job_accidental_stride")    # the reverse: a later job's own flags would differ from the launch's
    return L


def gcase(name, jobs, placing="aligned", role=None, *want):
    c = case(name, (), *want)
    c["jobs"], c["placing"], c["role"] = list(jobs), placing, role
    return c


_P = chain_products(65, 72, 63)          # n = 65, ckk = 72, P = 63: every product with a tail in M, N and K
_Q = chain_products(18, 33, 129, 2)
GEMM_CASES = [
    # the six products in their real orientations, each in a group of its own kind as the chain launches them
    gcase("role_HX", [chain_products(65, 72, 63, 3)["HX"], _Q["HX"]], "aligned", "HX", "kernel_kk", "splits_3_short_last", "splits_2", "k_72"),
    gcase("role_OUT", [_P["OUT"], _Q["OUT"], chain_products(64, 32, 1)["OUT"]], "offset", "OUT", "kernel_kn", "later_job_accidental_stride"),
    gcase("role_GH", [_P["GH"], _Q["GH"]], "exact", "GH", "kernel_mn", "m_65", "m_18"),
    gcase("role_DX", [_P["DX"], _Q["DX"]], "aligned", "DX", "kernel_mn", "m_63", "m_129"),
    gcase("role_gW1", [_P["gW1"], _Q["gW1"]], "offset", "gW1", "kernel_kk", "ep_add", "m_18"),
    gcase("role_gW", [_P["gW"], _Q["gW"]], "exact", "gW", "kernel_kn", "ep_add"),
    # the instantiation nothing in the library launches: A m-contiguous, B k-contiguous
    gcase("orient_mk", [gjob(65, 63, 33, "mk"), gjob(18, 129, 31, "mk", add=True)], "offset", None, "kernel_mk"),
    # sizes: M, N from {1, 18, 63, 64, 65, 129}, K from {1, 31, 32, 33, 72}
    gcase("sizes_a", [gjob(1, 129, 1, "kn"), gjob(129, 1, 31, "kn"), gjob(64, 64, 32, "kn"), gjob(63, 65, 33, "kn")], "aligned", None,
          "m_1", "n_1", "m_129", "n_129", "k_1", "k_31", "k_32", "k_33", "m_64", "n_64", "jobs_4"),
    gcase("sizes_b", [gjob(18, 18, 72, "kk"), gjob(65, 63, 32, "kk", add=True)], "exact", None, "n_18", "n_63", "m_65", "k_72"),
    gcase("one_job", [gjob(64, 65, 72, "mn", 2)], "aligned", None, "jobs_1", "splits_2"),
    # stores into NaN with ldc > N: the padding stays NaN; accumulation onto random contents with ldc > N
    gcase("ldc", [gjob(65, 63, 33, "kn", pad=5), gjob(18, 64, 31, "kn", add=True, pad=1), gjob(1, 1, 72, "kn", pad=3)], "offset", None,
          "ldc_gt_n", "jobs_3"),
    # a job without blocks first, in the middle (between jobs with blocks) and last
    gcase("zero_first", [gjob(0, 64, 32, "kn"), gjob(65, 18, 33, "kn"), gjob(18, 65, 31, "kn")], "aligned", None, "zero_first"),
    gcase("zero_middle", [gjob(63, 65, 72, "kk", 3), gjob(64, 0, 32, "kk"), gjob(0, 0, 1, "kk"), gjob(65, 129, 33, "kk")], "aligned", None,
          "zero_middle", "zero_between_live", "splits_3_short_last"),
    gcase("zero_last", [gjob(129, 18, 31, "mn"), gjob(64, 0, 32, "mn")], "exact", None, "zero_last", "jobs_2"),
    # job 0 at P = 1 (OUT: B = HY[n][1] has sBk = P = 1 by accident -> the kk kernel) and later jobs in the natural kn
    # orientation; and the reverse (the role_OUT case above also ends in one)
    gcase("p1_first", [chain_products(64, 72, 1)["OUT"], chain_products(65, 72, 65)["OUT"], chain_products(32, 72, 64)["OUT"]], "aligned",
          "OUT", "job0_accidental_flags", "kernel_kk", "n_1"),
    # GH with job 0 at P = 1: D[18][1] has a unit k stride by accident, and the launch is the <false, true> instantiation
    gcase("p1_first_gh", [chain_products(64, 72, 1)["GH"], chain_products(65, 72, 65)["GH"]], "aligned", "GH", "job0_accidental_flags",
          "kernel_mk"),
    gcase("p1_later",[chain_products(65, 72, 65)["GH"], chain_products(64, 72, 1)["GH"], chain_products(129, 72, 1)["GH"]], "offset",
          "GH", "later_job_accidental_stride", "kernel_mn"),
]
GEMM_REQUIRED = ({"role_" + r for r in ("HX", "OUT", "GH", "DX", "gW1", "gW")} | {"kernel_kk", "kernel_kn", "kernel_mn", "kernel_mk"} |
                 {"m_%d" % v for v in GEMM_M_N} | {"n_%d" % v for v in GEMM_M_N} | {"k_%d" % v for v in GEMM_K} |
                 {"splits_1", "splits_2", "splits_3_short_last", "last_split_short", "ep_store", "ep_add", "ldc_gt_n", "jobs_1",
                  "jobs_2", "jobs_3", "jobs_4", "zero_first", "zero_middle", "zero_between_live", "zero_last",
                  "job0_accidental_flags", "later_job_accidental_stride", "m_tail", "n_tail", "k_tail"})
# refused before any launch: (jobs, what)
GEMM_ERRORS = [
    ([], "no job"),
    ([gjob(8, 8, 32, "kn")] * 5, "five jobs"),
    ([gjob(64, 64, 64, "kk", 3)], "K = 64 in 3 splits: runs of 32, the third empty"),
    ([gjob(8, 8, 32, "kn"), gjob(18, 18, 33, "kn", 3)], "K = 33 in 3 splits, in the second job"),
]


def gemm_inputs(c):
    """-> per job dict(A, B, C0) in fp32: A and B dense in the job's orientation, C0 [M][ldc] random where the job adds, NaN
    where it stores (slabs: [splits][M][N] NaN)"""
    rng = rng_of("gemm_group", c["name"])
    out = []
    for j in c["jobs"]:
        M, N, K = j["M"], j["N"], j["K"]
        A = rng.randn(M, K).astype(np.float32)          # logical [M][K]
        B = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)   # logical [K][N]
        if j["splits"] > 1:
            C0 = np.full((j["splits"], M, N), np.nan, np.float32)
        else:
            C0 = rng.randn(M, N + j["pad"]).astype(np.float32) if j["add"] else np.full((M, N + j["pad"]), np.nan, np.float32)
            if j["add"]:
                C0[:, N:] = np.nan
        out.append(dict(A=A, B=B, C0=C0))
    return out


def gemm_layout(j, A, B):
    """the arrays as they lie in memory for the job's orientation"""
    a = A if j["orient"][0] == "k" else np.ascontiguousarray(A.T)
    b = np.ascontiguousarray(B.T) if j["orient"][1] == "k" else B
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def gemm_reference(j, d):
    """-> (want, mag, K of each compared block): unsplit want[M][N] (+ the old contents), split want[s][M][N]"""
    A, B = d["A"].astype(np.float64), d["B"].astype(np.float64)
    M, N = j["M"], j["N"]
    if j["splits"] > 1:
        kper, runs = k_runs(j["K"], j["splits"])
        want = np.stack([A[:, s * kper:s * kper + r] @ B[s * kper:s * kper + r] for s, r in enumerate(runs)])
        mag = np.stack([np.abs(A[:, s * kper:s * kper + r]) @ np.abs(B[s * kper:s * kper + r]) for s, r in enumerate(runs)])
        return want, mag, runs
    want, mag = A @ B, np.abs(A) @ np.abs(B)
    if j["add"]:
        want = want + d["C0"][:, :N]
        mag = mag + np.abs(d["C0"][:, :N].astype(np.float64))
    return want, mag, [j["K"]]


# ---- the chain: nets, positions, cases ---------------------------------------------------------------------------------------
def net(Cin, H, W, k, n, P, pos="corners", gin=True, force=0):
    Ho, Wo = H - k + 1, W - k + 1
    assert 0 <= P <= Ho * Wo
    return dict(Cin=Cin, H=H, W=W, k=k, n=n, P=P, Ho=Ho, Wo=Wo, ckk=Cin * k * k, pos=pos, gin=gin, force=force)


def positions(t, rng):
    """distinct positions inside the output map.  "corners": the four corners (as many as P allows, the last one first) and
    random others, in random order -- unsorted; "runs": two runs of adjacent positions, the second before the first in memory, so
    that up to k k patches overlap; "all": every position, shuffled (P = Ho Wo)"""
    hw, P, Wo = t["Ho"] * t["Wo"], t["P"], t["Wo"]
    if P == 0:
        return np.zeros(0, np.int32)
    if t["pos"] == "all":
        assert P == hw
        return rng.permutation(hw).astype(np.int32)
    if t["pos"] == "runs":
        a = P // 2
        s0 = int(rng.randint(0, hw - P + 1))
        run = np.arange(s0, s0 + P)
        return np.concatenate([run[a:], run[:a]]).astype(np.int32)
    corners = [hw - 1, 0, Wo - 1, hw - Wo][:min(P, 4)]
    rest = np.setdiff1d(np.arange(hw), corners)
    pick = list(corners) + list(rng.choice(rest, P - len(corners), replace=False))
    if P > 4:
        pick = list(rng.permutation(pick))
    return np.asarray(pick, np.int32)


def planned_splits(t):
    return t["force"] or head_splits(t["n"], t["Cin"], t["k"], t["P"])


def ccase(name, nets, *want, **kw):
    c = case(name, (), *want)
    c["nets"] = list(nets)
    c["exact"] = kw.get("exact", False)           # also run on small-integer data, compared bit for bit
    c["forward_only"] = kw.get("forward_only", False)
    return c


def _mixed(P, gin=(True, True, True, True), pos=("corners", "runs", "corners", "runs")):
    """four nets, k = (3, 3, 5, 7), widths that differ with one no multiple of 64, maps a few pixels larger than the kernel"""
    geo = ((8, 11, 12, 3, 64), (12, 12, 11, 3, 96), (16, 12, 13, 5, 32), (16, 15, 16, 7, 130))
    return [net(*(g + (p,)), pos=q, gin=gi) for g, p, gi, q in zip(geo, P, gin, pos)]


CHAIN_CASES = [
    ccase("mixed", _mixed((65, 1, 0, 64)), "p_1", "p_64", "p_65", "p_0_skipped", "n_differ", "act_backward_early_exit", "splits_3",
          exact=True),
    ccase("mixed_p1_first", _mixed((1, 65, 0, 64)), "p1_first", exact=True),
    ccase("mixed_p0_first", _mixed((0, 64, 65, 1)), "p0_first", exact=True),
    ccase("gin_null", _mixed((65, 64, 1, 64), gin=(True, False, True, False)), "gin_null_beside", exact=True),
    ccase("no_gin", _mixed((1, 65, 0, 64), gin=(False,) * 4), "no_gin"),
    ccase("forward_only", _mixed((65, 1, 0, 64)), "forward_only", forward_only=True),
    ccase("tiny_all", [net(8, 5, 6, 3, 18, 12, "all"), net(8, 7, 7, 7, 65, 1, "all")], "pos_all", exact=True),
    # P ckk = 1.2 M > 4096 x 256: im2col and col2im run their grid-stride loops; 8 splits of 320 with 112 left
    ccase("stride", [net(48, 29, 30, 7, 64, 512, "runs")], "grid_stride_col", "splits_8", "last_split_short", "fold_unrolled"),
    # 9 splits: the 8-wide fold and a tail of one; a forced count: 11 = 8 + 3
    ccase("fold", [net(48, 29, 30, 7, 64, 64, "corners")], "splits_9", "fold_unrolled_tail"),
    ccase("fold_forced_11", [net(48, 29, 30, 7, 64, 64, "corners", force=11)], "splits_11_forced", "fold_unrolled_tail"),
]
# the 4096-block cap of hd_grid for the [n][P] and [18][P] kernels needs n P (18 P) above 4096 x 256 = 1 048 576 elements: with
# P <= 4096 that is n > 256 at full P, and 18 P never gets there.  No shape is invented for it.
CHAIN_NOT_REACHED = {"grid_cap_nP", "grid_cap_18P"}
CHAIN_REQUIRED = {"p_1", "p_64", "p_65", "p_0_skipped", "p1_first", "p0_first", "n_differ", "n_not_multiple_64",
                  "act_backward_early_exit", "k_3", "k_5", "k_7", "pos_corners", "pos_runs", "pos_all", "pos_unsorted",
                  "patches_overlap_kk", "grid_stride_col", "splits_1", "splits_3", "splits_8", "splits_9", "splits_11_forced",
                  "last_split_short", "fold_tail_only", "fold_unrolled", "fold_unrolled_tail", "gin_null_beside", "no_gin",
                  "forward_only", "exact", "launches_fwd_5", "launches_bwd_7", "launches_bwd_5"}
# refused when the table is built: (net, what)
CHAIN_ERRORS = [
    (net(48, 29, 30, 7, 64, 64, force=12), "12 forced splits of K = 2352: runs of 224, eleven of them"),
    (net(48, 29, 30, 7, 64, 64, force=80), "80 forced splits: runs of 32, 74 of them"),
]


def overlaps_kk(t):
    """some element of the input map lies under k k patches: the positions hold k full rows of an output map k wide or more (a
    run of L adjacent positions holds at least (L - Wo + 1) // Wo full rows)"""
    rows = t["Ho"] if t["pos"] == "all" else (t["P"] - t["Wo"] + 1) // t["Wo"] if t["pos"] == "runs" else 0
    return t["Wo"] >= t["k"] and rows >= t["k"]


def chain_labels(c):
    L = set()
    nets = c["nets"]
    live = [t for t in nets if t["P"] > 0]
    for t in nets:
        if t["P"] == 0:
            L.add("p_0_skipped")
    if nets[0]["P"] == 0:
        L.add("p0_first")
    if nets[0]["P"] == 1 and any(t["P"] > 1 for t in nets[1:]):
        L.add("p1_first")
    if len({t["n"] for t in live}) > 1:
        L.add("n_differ")
        L.add("act_backward_early_exit")        # blockIdx.x runs to the widest net: c >= j.n in the others
    for t in live:
        if t["P"] in (1, 64, 65):
            L.add("p_%d" % t["P"])
        if t["n"] % 64:
            L.add("n_not_multiple_64")
        L.add("k_%d" % t["k"])
        L.add("pos_" + t["pos"])
        if t["pos"] == "corners" and t["P"] > 4:
            L.add("pos_unsorted")
        if overlaps_kk(t):
            L.add("patches_overlap_kk")
        if t["P"] * t["ckk"] > HD_GRID_CAP * 256:
            L.add("grid_stride_col")
        assert t["n"] * t["P"] <= HD_GRID_CAP * 256, "a shape for the cap of the [n][P] kernels: see CHAIN_NOT_REACHED"
        S = planned_splits(t)
        kper, runs = k_runs(t["ckk"], S)
        assert len(runs) == S and S * t["P"] <= SLAB_POSITIONS
        L.add("splits_%d%s" % (S, "_forced" if t["force"] else ""))
        if S > 1 and runs[-1] < kper:
            L.add("last_split_short")
        L.add("fold_tail_only" if S < 8 else "fold_unrolled" if S % 8 == 0 else "fold_unrolled_tail")
    if live:
        L.add("launches_fwd_5")
        if c["forward_only"]:
            L.add("forward_only")
        elif any(t["gin"] for t in live):
            L.add("launches_bwd_7")
            if any(not t["gin"] for t in live):
                L.add("gin_null_beside")
        else:
            L.add("launches_bwd_5")
            L.add("no_gin")
    if c["exact"]:
        L.add("exact")
    return L


SLOPE = {False: 0.1, True: 0.25}    # exact data: a power of two


def net_data(c, i, exact=False):
    """the tensors of net i of a case, fp32: inputs, parameters, the delta map (zero off the positions), and what the
    accumulating destinations hold before the backward pass.  exact: small integers (multiples of 1/4 once the slope has acted),
    sparse enough that every sum of magnitudes stays below 2^22: see exact_condition."""
    t = c["nets"][i]
    rng = rng_of("heads_chain", c["name"], i, exact)
    n, ckk, hw = t["n"], t["ckk"], t["Ho"] * t["Wo"]
    pos = positions(t, rng)
    shape_in = (t["Cin"], t["H"], t["W"])
    if exact:
        ints = lambda lo, hi, shape, keep=1.0: (rng.randint(lo, hi + 1, size=shape) * (rng.rand(*shape) < keep)).astype(np.float32)   # noqa: E731
        d = dict(inp=ints(-2, 2, shape_in), w3=ints(-1, 1, (n, ckk), 0.25), bias3=ints(-2, 2, (n,)), w1=ints(-1, 1, (HEAD_OUT, n), 0.5),
                 bias1=ints(-2, 2, (HEAD_OUT,)), gin0=ints(-3, 3, shape_in), gw3_0=ints(-3, 3, (n, ckk)), gbias3_0=ints(-3, 3, (n,)),
                 gw1_0=ints(-3, 3, (HEAD_OUT, n)), gbias1_0=ints(-3, 3, (HEAD_OUT,)), gslope0=np.float32(rng.randint(-3, 4)))
        dv = ints(-2, 2, (HEAD_OUT, t["P"]), 0.25)
    else:
        d = dict(inp=rng.randn(*shape_in).astype(np.float32), w3=(rng.randn(n, ckk) / np.sqrt(ckk)).astype(np.float32),
                 bias3=(0.1 * rng.randn(n)).astype(np.float32), w1=(rng.randn(HEAD_OUT, n) / np.sqrt(n)).astype(np.float32),
                 bias1=(0.1 * rng.randn(HEAD_OUT)).astype(np.float32), gin0=rng.randn(*shape_in).astype(np.float32),
                 gw3_0=rng.randn(n, ckk).astype(np.float32), gbias3_0=rng.randn(n).astype(np.float32),
                 gw1_0=rng.randn(HEAD_OUT, n).astype(np.float32), gbias1_0=rng.randn(HEAD_OUT).astype(np.float32),
                 gslope0=np.float32(rng.randn()))
        dv = rng.randn(HEAD_OUT, t["P"]).astype(np.float32)
    d["slope"] = np.float32(SLOPE[exact])
    d["pos"] = pos
    delta = np.zeros((HEAD_OUT, hw), np.float32)
    delta[:, pos] = dv
    d["delta"] = delta
    return d


# ---- fp64 references, stage by stage (every function takes the stage before it, so that the GPU test can feed the device's) ----
def f64(a):
    return np.asarray(a, np.float64)


def ref_col(t, inp, pos):
    """COL[p][(c, ky, kx)] = in[c][y_p + ky][x_p + kx] (any dtype: a pure move)"""
    k, Wo = t["k"], t["Wo"]
    out = np.empty((len(pos), t["ckk"]), inp.dtype)
    for p, q in enumerate(pos):
        y, x = divmod(int(q), Wo)
        out[p] = inp[:, y:y + k, x:x + k].reshape(-1)
    return out


def ref_slabs(w3, COL, S):
    """-> (slabs[S][n][P], mag likewise, run lengths)"""
    ckk = w3.shape[1]
    kper, runs = k_runs(ckk, S)
    W, X = f64(w3), f64(COL)
    sl = np.stack([W[:, s * kper:s * kper + r] @ X[:, s * kper:s * kper + r].T for s, r in enumerate(runs)])
    mg = np.stack([np.abs(W[:, s * kper:s * kper + r]) @ np.abs(X[:, s * kper:s * kper + r]).T for s, r in enumerate(runs)])
    return sl, mg, runs


def ref_hx(bias3, slabs):
    return f64(bias3)[:, None] + f64(slabs).sum(0), np.abs(f64(bias3))[:, None] + np.abs(f64(slabs)).sum(0)


def ref_hy(HX, slope):
    HX = f64(HX)
    return np.where(HX > 0, HX, float(slope) * HX)


def ref_out(w1, HY):
    return f64(w1) @ f64(HY), np.abs(f64(w1)) @ np.abs(f64(HY))


def ref_gh(w1, D, HX, slope):
    """GH = (w1^T D) prelu'(HX) -> (GH, mag, GH0 = w1^T D, mag0)"""
    g0, m0 = f64(w1).T @ f64(D), np.abs(f64(w1)).T @ np.abs(f64(D))
    f = np.where(f64(HX) > 0, 1.0, float(slope))
    return g0 * f, m0 * np.abs(f), g0, m0


def ref_gslope(HX, GH0, mag0):
    neg = ~(f64(HX) > 0)
    return float((f64(HX) * GH0)[neg].sum()), float((np.abs(f64(HX)) * mag0)[neg].sum())


def ref_col2im(t, DX, pos, gin0):
    """-> (gin, mag, patches covering each element)"""
    k, Wo = t["k"], t["Wo"]
    g, m, cnt = f64(gin0).copy(), np.abs(f64(gin0)), np.zeros(gin0.shape, np.int64)
    D = f64(DX).reshape(len(pos), t["Cin"], k, k)
    for p, q in enumerate(pos):
        y, x = divmod(int(q), Wo)
        g[:, y:y + k, x:x + k] += D[p]
        m[:, y:y + k, x:x + k] += np.abs(D[p])
        cnt[:, y:y + k, x:x + k] += 1
    return g, m, cnt


def reference(t, d):
    """the whole chain in fp64 from the inputs: forward, and the backward pass onto the *_0 contents"""
    pos, slope = d["pos"], float(d["slope"])
    r = dict(COL=ref_col(t, f64(d["inp"]), pos))
    r["HX"] = f64(d["w3"]) @ r["COL"].T + f64(d["bias3"])[:, None]
    r["HY"] = ref_hy(r["HX"], slope)
    r["OUT"] = f64(d["w1"]) @ r["HY"]
    r["out_at_pos"] = r["OUT"] + f64(d["bias1"])[:, None]
    r["D"] = f64(d["delta"])[:, pos]
    r["gbias1"] = f64(d["gbias1_0"]) + r["D"].sum(1)
    r["GH"], _, g0, _ = ref_gh(d["w1"], r["D"], r["HX"], slope)
    r["gbias3"] = f64(d["gbias3_0"]) + r["GH"].sum(1)
    r["gslope"] = float(d["gslope0"]) + ref_gslope(r["HX"], g0, np.abs(g0))[0]
    r["DX"] = r["GH"].T @ f64(d["w3"])
    r["gin"] = ref_col2im(t, r["DX"], pos, d["gin0"])[0]
    r["gw1"] = f64(d["gw1_0"]) + r["D"] @ r["HY"].T
    r["gw3"] = f64(d["gw3_0"]) + r["GH"] @ r["COL"]
    return r


def exact_condition(t, d):
    """-> the largest sum of magnitudes, in units of 1/4, that any accumulation of the chain can reach on the data d, whatever
    its order: every stage on magnitudes.  Below 2^24 every partial sum is a multiple of 1/4 (the slope is 1/4, everything else an
    integer) of fewer than 24 bits: fp32 holds it exactly, so the device must give the fp64 reference bit for bit."""
    a = lambda x: np.abs(f64(x))   # noqa: E731
    pos, s = d["pos"], float(d["slope"])
    assert s == 0.25
    for v in d.values():
        assert np.array_equal(np.asarray(v, np.float64) * 4, np.round(np.asarray(v, np.float64) * 4))
    COL = ref_col(t, a(d["inp"]), pos)
    HX = a(d["w3"]) @ COL.T + a(d["bias3"])[:, None]
    OUT = a(d["w1"]) @ HX + a(d["bias1"])[:, None]          # (|HY| <= |HX|)
    D = a(d["delta"])[:, pos]
    GH = a(d["w1"]).T @ D
    worst = [HX.max(), OUT.max(), (a(d["gbias1_0"]) + D.sum(1)).max(), GH.max(), (a(d["gbias3_0"]) + GH.sum(1)).max(),
             abs(float(d["gslope0"])) + (HX * GH).sum(), (a(d["gw1_0"]) + D @ HX.T).max(), (a(d["gw3_0"]) + GH @ COL).max()]
    DX = GH.T @ a(d["w3"])
    worst += [DX.max(), ref_col2im(t, DX, pos, a(d["gin0"]))[0].max()]
    return 4.0 * max(worst)


# ---- the dense restatement the host test anchors the references with ----------------------------------------------------------
def dense_forward(t, d):
    """fp64 valid convolution, PReLU, 1 x 1 convolution on the WHOLE map -> (hx[n][Ho][Wo], hy, out[18][Ho][Wo])"""
    k, Ho, Wo = t["k"], t["Ho"], t["Wo"]
    x, w = f64(d["inp"]), f64(d["w3"]).reshape(t["n"], t["Cin"], k, k)
    hx = np.zeros((t["n"], Ho, Wo)) + f64(d["bias3"])[:, None, None]
    for ky in range(k):
        for kx in range(k):
            hx += np.einsum("oc,cyx->oyx", w[:, :, ky, kx], x[:, ky:ky + Ho, kx:kx + Wo])
    hy = np.where(hx > 0, hx, float(d["slope"]) * hx)
    out = np.einsum("on,nyx->oyx", f64(d["w1"]), hy) + f64(d["bias1"])[:, None, None]
    return hx, hy, out


def dense_backward(t, d):
    """the dense backward pass of the same net with the delta map as it is (zero off the positions), added to the *_0 contents"""
    k, Ho, Wo, n = t["k"], t["Ho"], t["Wo"], t["n"]
    hx, hy, _ = dense_forward(t, d)
    delta = f64(d["delta"]).reshape(HEAD_OUT, Ho, Wo)
    x, w = f64(d["inp"]), f64(d["w3"]).reshape(n, t["Cin"], k, k)
    g = dict(gbias1=f64(d["gbias1_0"]) + delta.sum((1, 2)), gw1=f64(d["gw1_0"]) + np.einsum("oyx,nyx->on", delta, hy))
    ghy = np.einsum("on,oyx->nyx", f64(d["w1"]), delta)
    ghx = np.where(hx > 0, ghy, float(d["slope"]) * ghy)
    g["gslope"] = float(d["gslope0"]) + float((hx * ghy)[~(hx > 0)].sum())
    g["gbias3"] = f64(d["gbias3_0"]) + ghx.sum((1, 2))
    gw = np.zeros_like(w)
    gin = f64(d["gin0"]).copy()
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = np.einsum("oyx,cyx->oc", ghx, x[:, ky:ky + Ho, kx:kx + Wo])
            gin[:, ky:ky + Ho, kx:kx + Wo] += np.einsum("oc,oyx->cyx", w[:, :, ky, kx], ghx)
    g["gw3"] = f64(d["gw3_0"]) + gw.reshape(n, -1)
    g["gin"] = gin
    return g


def find(name):
    for c in GEMM_CASES + CHAIN_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)
