"""The case tables of tests/test_gpu_gemm_plans.py and a plain restatement of the host-side shape rules of the two files
that compute every nn.Linear of the classification net: csrc/gemm.hip (gemm_f32: the fp32 matrix-core product) and
csrc/gemmx.hip (gx_plan / gx_run / gemm_planes_kernel: the split-operand product), for the three products of
Linear(R rows, I inputs, O outputs) as csrc/linear.h issues them -- for the entry points frcnn_linear_forward /
frcnn_linear_backward, which the GPU cases call, and for the classification net alike: both run that one header.

As in tests/conv_plan.py, tests/convx_plan.py, tests/width_plan.py and tests/cnet_plan.py the restatement only LABELS the
GPU cases with the branches they reach, so that tests/test_gemm_plan.py can check that the tables still reach every one of
them: it is no evidence that a branch computes the right thing.  The GPU tests against the fp64 references are.

Shapes are written (R, I, O).  The three products:
  forward          Y[R][O]   = X[R][I] W[O][I]^T + b   M = R, N = O, K = I   A k-contiguous, B k-contiguous, bias, store
  input gradient   gX[R][I]  = gY[R][O] W[O][I]        M = R, N = I, K = O   A k-contiguous, B n-contiguous, store
  weight gradient  gW[O][I] += gY[R][O]^T X[R][I]      M = O, N = I, K = R   A m-contiguous, B n-contiguous, accumulate
The fourth orientation of gemm_f32 (A m-contiguous, B k-contiguous) has no caller in the library: its four register
instantiations and its DMA instantiation are compiled and never launched, and no case here can reach them."""
import cnet_plan as NP
import width_plan as WP
from conv_plan import case
from width_plan import cdiv

ROLES = ("forward", "input_gradient", "weight_gradient")
SHORT = {"forward": "fwd", "input_gradient": "dgrad", "weight_gradient": "wgrad"}
ROLE_BIT = {"forward": 1, "input_gradient": 2, "weight_gradient": 4}

# ---- gemm.hip: gemm_f32 ----------------------------------------------------------------------------------------------------
GBK = NP.GBK        # K values per block step of both kernels (GD_BK is the same 32)
EDGE_SIZES = (1, 4, 63, 64, 65)


def f32_product(role, R, I, O):
    """the call linear.h makes: M, N, K, the four strides, and what becomes of the result"""
    if role == "forward":
        return dict(M=R, N=O, K=I, sAm=I, sAk=1, sBk=1, sBn=I, bias=True, add=False, a="x", b="w")
    if role == "input_gradient":
        return dict(M=R, N=I, K=O, sAm=O, sAk=1, sBk=I, sBn=1, bias=False, add=False, a="gy", b="w")
    return dict(M=O, N=I, K=R, sAm=1, sAk=O, sBk=I, sBn=1, bias=False, add=True, a="gy", b="x")


def f32_plan(role, shape, a_aligned=True, b_aligned=True):
    """gemm.hip gemm_f32.  a_aligned / b_aligned: the operand starts on 16 bytes (else 4 bytes off: every tensor of the
    library is a multiple of 4 bytes into its allocation)."""
    R, I, O = shape
    q = f32_product(role, R, I, O)
    M, N, K = q["M"], q["N"], q["K"]
    s = NP.gemm_split_plan(M, N, K)
    kPer, splitK = s["kPerSplit"], s["splitK"]
    ak, bk = q["sAk"] == 1, q["sBk"] == 1

    def vec_ok(aligned, kc, sRow, sK, nRows):
        if not aligned:
            return False
        if kc:
            return sK == 1 and sRow % 4 == 0 and K % 4 == 0 and kPer % 4 == 0
        return sRow == 1 and sK % 4 == 0 and nRows % 4 == 0

    def chunk_ok(kc, sRow, sK, nRows):
        if kc:
            return sK == 1 and K % 4 == 0 and kPer % 4 == 0
        return sRow == 1 and nRows % 4 == 0
    av, bv = vec_ok(a_aligned, ak, q["sAm"], q["sAk"], M), vec_ok(b_aligned, bk, q["sBn"], q["sBk"], N)
    ad, bd = chunk_ok(ak, q["sAm"], q["sAk"], M), chunk_ok(bk, q["sBn"], q["sBk"], N)
    dma = (ad and bd and (kPer % GBK == 0 or splitK == 1) and K >= 64 and (ak or (M % 4 == 0 and M >= 4)) and
           (bk or (N % 4 == 0 and N >= 4)))
    last = K - (splitK - 1) * kPer
    if splitK > 1:
        where = "fold_bias" if q["bias"] else "fold_accumulate" if q["add"] else "fold"
    else:
        where = "tile_accumulate" if q["add"] else "tile_store"
    return dict(role=role, M=M, N=N, K=K, TNs=s["TNs"], tiles=s["tiles"], by_k=s["by_k"], by_slots=s["by_slots"],
                estimate=s["estimate"], kPerSplit=kPer, splitK=splitK, last=last, ak=ak, bk=bk, av=av, bv=bv, dma=dma,
                where=where, bias=q["bias"])


def f32_labels(p):
    """labels of one gemm_f32 launch; each also with the role in front ("dgrad:tn128_reg")"""
    L = set()
    orient = ("k" if p["ak"] else "m") + ("k" if p["bk"] else "n")
    kernel = "dma" if p["dma"] else "reg"
    L.add("tn%d_%s" % (p["TNs"], kernel))
    L.add("dma_" + orient if p["dma"] else "reg_%s_%d%d" % (orient, p["av"], p["bv"]))
    S = p["splitK"]
    L.add("splits_1" if S == 1 else "splits_2_8" if S <= 8 else "splits_9_16")
    if S > 1:
        if p["by_slots"] < p["by_k"]:
            L.add("splits_capped_by_slots")
        if p["last"] < p["kPerSplit"]:
            L.add("last_split_short")
        if S < p["estimate"]:
            L.add("splits_recomputed")
        if p["last"] % GBK:
            L.add("k_tail_last_split")
            L.add("k_tail_last_split_" + kernel)
    elif p["K"] % GBK:
        L.add("k_tail_unsplit")
        L.add("k_tail_unsplit_" + kernel)
    if p["K"] < 64:
        L.add("k_lt_64")
    L.add("ep_" + p["where"])
    if p["where"] == "tile_store" and p["bias"]:
        L.add("ep_tile_bias")
    for n in EDGE_SIZES:
        if p["M"] == n:
            L.add("m_%d" % n)
        if p["N"] == n:
            L.add("n_%d" % n)
    if p["M"] % 64:
        L.add("m_tail")
    if p["N"] % p["TNs"]:
        L.add("n_tail")
    return L | {"%s:%s" % (SHORT[p["role"]], l) for l in L}


# where the tensors of a run lie (tests/test_gpu_convx_plans.py::Placed): "slack" = at the start of an allocation with room
# behind it, "offset" = 4 bytes into one, "exact" = ending where its allocation ends.  Tensors not named lie at "slack".
PLACINGS = {
    "aligned": {},
    "x_offset": dict(x="offset"),
    "w_offset": dict(w="offset"),
    "offset": dict(x="offset", w="offset", gy="offset", b="offset", y="offset", gx="offset", gw="offset", gb="offset"),
    "exact": dict(x="exact", w="exact", gy="exact", b="exact", y="exact", gx="exact", gw="exact", gb="exact"),
}


def fcase(name, shape, placings, *want, **kw):
    c = case(name, shape, *want)
    c["placings"] = tuple(placings)
    c["roles"] = tuple(kw.get("roles", ROLES))
    return c


ALL = ("aligned", "offset", "exact")
F32_CASES = [
    # the shapes the launcher's rules were read for, one line of the table each
    fcase("tn128", (5, 2304, 2050), ALL, "fwd:tn128_dma", "fwd:splits_9_16", "fwd:ep_fold_bias", "dgrad:tn128_reg",
          "dgrad:reg_kn_01", "dgrad:splits_2_8", "dgrad:last_split_short", "dgrad:k_tail_last_split_reg", "wgrad:reg_mn_01",
          "wgrad:k_lt_64", "wgrad:ep_tile_accumulate"),
    fcase("fold_accumulate", (600, 2052, 520), ALL, "fwd:splits_2_8", "fwd:last_split_short", "fwd:k_tail_last_split_dma",
          "dgrad:tn128_dma", "dgrad:dma_kn", "dgrad:ep_fold", "wgrad:tn128_dma", "wgrad:dma_mn", "wgrad:ep_fold_accumulate"),
    fcase("bbox_head", (65, 4100, 4), ALL, "fwd:splits_9_16", "fwd:splits_recomputed", "fwd:last_split_short", "fwd:n_4",
          "fwd:m_65", "dgrad:k_lt_64", "dgrad:reg_kn_11", "wgrad:m_4", "wgrad:dma_mn", "wgrad:k_tail_unsplit_dma"),
    fcase("wgrad_four_slabs", (1030, 68, 36), ("aligned", "exact"), "wgrad:splits_2_8", "wgrad:last_split_short",
          "wgrad:ep_fold_accumulate", "fwd:dma_kk", "fwd:ep_tile_bias"),
    # K < 64 with every operand divisible by 4: the register kernel by size; which operand is 16-byte aligned picks the loads
    fcase("short_k", (64, 60, 64), ("aligned", "x_offset", "w_offset", "offset"), "fwd:k_lt_64", "fwd:reg_kk_11",
          "fwd:reg_kk_10", "fwd:reg_kk_01", "fwd:reg_kk_00", "fwd:m_64", "fwd:n_64", "wgrad:dma_mn"),
    fcase("sixteen_slabs", (3, 8200, 65), ("aligned", "exact"), "fwd:splits_9_16", "fwd:n_65", "fwd:last_split_short",
          roles=("forward",)),
    fcase("wgrad_tn128_tail", (513, 2048, 20), ("aligned", "exact"), "wgrad:tn128_dma", "wgrad:k_tail_last_split_dma",
          "wgrad:ep_fold_accumulate", roles=("weight_gradient",)),
    # the split estimate capped by the resident slots (2048 / 729 tiles = 2) and not by K / 256 = 3
    fcase("capped_by_slots", (1665, 768, 1666), ("aligned",), "fwd:splits_capped_by_slots", "fwd:splits_2_8",
          roles=("forward",)),
    # edge sizes of M and N and the register variants the divisibility of I and O decides
    fcase("one_row", (1, 100, 63), ALL, "fwd:m_1", "fwd:n_63", "fwd:k_tail_unsplit_dma", "dgrad:reg_kn_01", "wgrad:m_63",
          "wgrad:reg_mn_01"),
    fcase("one_output", (63, 65, 1), ALL, "fwd:m_63", "fwd:n_1", "fwd:reg_kk_00", "fwd:k_tail_unsplit_reg", "dgrad:reg_kn_00",
          "dgrad:n_65", "wgrad:m_1"),
    fcase("tile_plus_one", (64, 64, 65), ALL, "fwd:n_65", "fwd:dma_kk", "dgrad:reg_kn_01", "dgrad:n_64", "wgrad:m_65",
          "wgrad:reg_mn_01"),
    fcase("row_past_tile", (65, 68, 64), ALL, "fwd:m_65", "dgrad:dma_kn", "wgrad:m_64", "wgrad:dma_mn", "wgrad:k_tail_unsplit_dma"),
    fcase("odd_inputs", (9, 70, 8), ALL, "dgrad:reg_kn_10", "wgrad:reg_mn_10", "fwd:reg_kk_00"),
    fcase("few_rows", (33, 72, 40), ALL, "wgrad:reg_mn_11", "dgrad:reg_kn_11", "fwd:dma_kk"),
    fcase("ragged", (70, 66, 33), ALL, "wgrad:reg_mn_00", "dgrad:reg_kn_00", "fwd:reg_kk_00"),
]

REG_VARIANTS = {"reg_%s_%d%d" % (o, a, b) for o in ("kk", "kn", "mn") for a in (0, 1) for b in (0, 1)}
F32_REQUIRED = REG_VARIANTS | {
    "tn64_dma", "tn128_dma", "tn64_reg", "tn128_reg",
    "splits_1", "splits_2_8", "splits_9_16", "splits_capped_by_slots", "splits_recomputed", "last_split_short",
    "k_tail_unsplit", "k_tail_last_split", "k_tail_unsplit_dma", "k_tail_unsplit_reg", "k_tail_last_split_dma",
    "k_tail_last_split_reg", "k_lt_64",
    "dma_kk", "dma_kn", "dma_mn",
    "ep_tile_store", "ep_tile_bias", "ep_tile_accumulate", "ep_fold", "ep_fold_accumulate", "ep_fold_bias",
    "m_tail", "n_tail",
} | {"m_%d" % n for n in EDGE_SIZES} | {"n_%d" % n for n in EDGE_SIZES}


def f32_runs(cases=None):
    """every test of the gemm_f32 part: (case, placing); a run issues the case's roles"""
    return [dict(name=c["name"], shape=c["shape"], placing=pl, roles=c["roles"])
            for c in (F32_CASES if cases is None else cases) for pl in c["placings"]]


def tensor_sizes(shape):
    R, I, O = shape
    return dict(x=R * I, w=O * I, b=O, gy=R * O, y=R * O, gx=R * I, gw=O * I, gb=O)


def starts_aligned(placing, tensor, shape):
    """the tensor starts on 16 bytes: at the start of its allocation, or ending with it (Placed asks for 8 floats more than the
    tensor has and gets exactly those: the tensor starts 32 bytes in; the GPU test asserts that the tensors lie as assumed)"""
    return PLACINGS[placing].get(tensor, "slack") != "offset"


def f32_plans_of_run(r):
    out = []
    for role in r["roles"]:
        q = f32_product(role, *r["shape"])
        out.append(f32_plan(role, r["shape"], starts_aligned(r["placing"], q["a"], r["shape"]),
                            starts_aligned(r["placing"], q["b"], r["shape"])))
    return out


def f32_labels_of_run(r):
    L = set()
    for p in f32_plans_of_run(r):
        L |= f32_labels(p)
    return L


# ---- gemmx.hip --------------------------------------------------------------------------------------------------------------
GX_TN = 256
GX_LDS_MAX = 160 * 1024
GX_TMS = (256, 192, 128, 64)
GX_WGRAD_SLAB_ROWS = 1024
FORMS = {0: "bf16x6", 1: "f16x3"}     # option x3_f16 -> the operand form
PLANES = {0: 3, 1: 2}


def linear_x_rows_padded(R):
    return (R + 15) & ~15


def linear_x_eligible(role, R, I, O, mask=-1, split_bf16=True):
    """gemmx.hip linear_x_eligible with option gemm_x_roles = mask (role: 1 forward, 2 input gradient, 4 weight gradient);
    mask = -1 is the built-in rule, width_plan.linear_x_eligible"""
    if mask < 0:
        return split_bf16 and WP.linear_x_eligible(role, R, I, O)
    if not split_bf16 or I % 16 or O % 16 or R < 32 or R * I * O < 1.0e9:
        return False
    return (mask & role) != 0


def gx_stage_bytes(TM, bmode, planes):
    return 32 * planes * TM + (32 * planes * GX_TN if bmode == 0 else 64 * GX_TN)


def gx_blocks_per_cu(TM):
    return 2 if TM <= 128 else 1


def gx_ring(TM, bmode, planes):
    room = (GX_LDS_MAX - (1024 if planes == 2 else 0)) // gx_blocks_per_cu(TM) // gx_stage_bytes(TM, bmode, planes)
    return max(2, min(4, room))


def gx_plan(M, N, K, bmode, splitK_min, splitK_max, forced_tm=None):
    """gemmx.hip gx_plan, its cost model term for term -> (TM, splits).  forced_tm: environment FRCNN_GX_TM; a height the
    operand form does not have (256 rows with fp32 weights) forces nothing."""
    best, TM, splitK = 1e300, 128, 1
    if forced_tm == 256 and bmode != 0:
        forced_tm = None
    for tmv in GX_TMS:
        if tmv == 256 and bmode != 0:
            continue
        if forced_tm is not None and forced_tm != tmv:
            continue
        tiles = cdiv(M, tmv) * cdiv(N, GX_TN)
        bpc = gx_blocks_per_cu(tmv)
        for sk in range(splitK_min, splitK_max + 1):
            kper = cdiv(cdiv(K, sk), 16) * 16
            if sk > 1 and kper < 256:
                break
            sk_eff = cdiv(K, kper)
            b = cdiv(tiles * sk_eff, 256)
            mf, steps, fixed = (tmv // 64) * 768.0, float(kper // 16), 8000.0 + 12.0 * tmv
            alone, paired = steps * (mf / 0.80 + 300.0) + fixed, steps * (2.0 * mf / 0.92 + 150.0) + fixed
            cost = (b // 2) * paired + (b % 2) * alone if bpc == 2 else b * alone
            if sk_eff > 1:
                cost += 8.0 * sk_eff * float(M) * N / 1500.0 / 8.0 + 6000.0
            if cost < best:
                best, TM, splitK = cost, tmv, sk_eff
    return TM, splitK


def gx_product(role, R, I, O):
    """gemmx.hip linear_x_forward / _dgrad / _wgrad: M, N, K, how B is read (0 planes, 1 fp32 k-contiguous, 2 fp32
    n-contiguous) and the fewest and most splits the role asks gx_plan for (the weight gradient: one slab per
    GX_WGRAD_SLAB_ROWS rows of k, no choice)"""
    if role == "forward":
        return dict(M=R, N=O, K=I, bmode=1, splitK_min=1, splitK_max=32, add=False)
    if role == "input_gradient":
        return dict(M=R, N=I, K=O, bmode=2, splitK_min=1, splitK_max=4, add=False)
    Rp = linear_x_rows_padded(R)
    splits = cdiv(Rp, GX_WGRAD_SLAB_ROWS)
    return dict(M=O, N=I, K=Rp, bmode=0, splitK_min=splits, splitK_max=splits, add=True)


def gx_launch(role, shape, form, forced_tm=None):
    """gemmx.hip gx_run for one role of Linear(R, I, O) in operand form `form` (option x3_f16)"""
    R, I, O = shape
    q = gx_product(role, R, I, O)
    M, N, K = q["M"], q["N"], q["K"]
    assert K % 16 == 0
    TM, splitK = gx_plan(M, N, K, q["bmode"], q["splitK_min"], q["splitK_max"], forced_tm)
    tm, tn = cdiv(M, TM), cdiv(N, GX_TN)
    kPer = cdiv(cdiv(K, splitK), 16) * 16
    splitK = cdiv(K, kPer)
    last = K - (splitK - 1) * kPer
    ring = gx_ring(TM, q["bmode"], PLANES[form])
    return dict(role=role, form=form, R=R, M=M, N=N, K=K, bmode=q["bmode"], TM=TM, tm=tm, tn=tn, splitK=splitK, kPerSplit=kPer,
                last=last, ring=ring, blocks=tm * tn * splitK, steps=kPer // 16, last_steps=last // 16, fold=splitK > 1,
                n=PLANES_PRODUCTS[form] * K)


PLANES_PRODUCTS = {0: 6, 1: 3}     # kept plane products per fp32 product (convx_plan.PRODUCTS)


def gx_labels(p):
    """labels of one gemm_planes_kernel launch: "<role>:<label>" and, for what depends on the form, "<form>:<label>"."""
    L = set()
    L.add("tm%d" % p["TM"])
    S = p["splitK"]
    L.add("splits_1" if S == 1 else "splits_2_8" if S <= 8 else "splits_gt_8")
    if S > 1:
        L.add("fold")
        if p["last"] < p["kPerSplit"]:
            L.add("last_split_short")
    if p["M"] < p["TM"]:
        L.add("m_lt_tm")
    if p["M"] % p["TM"]:
        L.add("m_mod_tm")
        if p["M"] % p["TM"] == 1:
            L.add("m_mod_tm_1")
    if p["N"] < GX_TN:
        L.add("n_lt_256")
    if p["N"] % GX_TN:
        L.add("n_mod256")
        L.add("n_mod256_%d" % (p["N"] % GX_TN))
    if p["role"] == "weight_gradient":
        if p["K"] == 32:
            L.add("rp_32")
        if p["K"] - p["R"] == 15:
            L.add("rp_15_zero_rows")
    F = set()
    if min(p["steps"], p["last_steps"]) < p["ring"]:
        F.add("steps_lt_ring")
    if min(p["steps"], p["last_steps"]) == p["ring"]:
        F.add("steps_eq_ring")
    if p["blocks"] % 8:
        F.add("blocks_mod8")
    if p["blocks"] < 8:
        F.add("blocks_lt_8")
    F.add("ring%d" % p["ring"])
    role, form = SHORT[p["role"]], FORMS[p["form"]]
    out = {"%s:%s" % (role, l) for l in L | F}
    out |= {"%s:%s" % (form, l) for l in F}
    out |= {"%s:%s" % (form, role)}
    return out


def xcase(name, shape, tms, *want, **kw):
    c = case(name, shape, *want)
    c["tms"] = tuple(tms)                        # FRCNN_GX_TM of each run; None = the planner's choice
    c["placing"] = kw.get("placing", "aligned")
    c["wide"] = kw.get("wide", False)            # also run with activation operands that span twelve binades
    return c


# Every case is eligible in all three roles under gemm_x_roles = 7 (R I O >= 1e9, I and O multiples of 16, R >= 32) and runs
# all three in both operand forms; within about 1.3e9 multiply-adds.
GX_CASES = [
    xcase("n_tail_16", (270, 13824, 272), (None,), "fwd:n_mod256_16", "fwd:splits_gt_8", "fwd:fold", "dgrad:m_mod_tm",
          placing="exact"),
    xcase("n_lt_256", (1100, 4112, 240), (None,), "fwd:n_lt_256", "fwd:n_mod256_240", "dgrad:n_mod256_16",
          placing="offset"),
    xcase("n_tail_224", (200, 6928, 736), (None,), "fwd:n_mod256_224", "dgrad:n_mod256_16"),
    xcase("n_tail_240", (2000, 1040, 496), (None,), "fwd:n_mod256_240", "fwd:splits_2_8", "dgrad:n_mod256_16", "wgrad:n_mod256",
          placing="exact"),
    xcase("short_last", (250, 2048, 2064), (None,), "fwd:splits_2_8", "fwd:last_split_short", "dgrad:splits_2_8",
          "dgrad:last_split_short", wide=True),
    xcase("few_rows", (40, 3088, 8208), (None,), "fwd:m_lt_tm", "dgrad:m_lt_tm", "dgrad:splits_2_8", "dgrad:last_split_short",
          "fwd:n_mod256_16", "dgrad:n_mod256_16"),
    xcase("rp_32", (32, 13824, 2304), (None, 256), "wgrad:rp_32", "wgrad:steps_lt_ring", "f16x3:steps_lt_ring", "wgrad:tm256",
          "fwd:m_lt_tm"),
    xcase("rp_48", (33, 13824, 2304), (None, 192), "wgrad:rp_15_zero_rows", "wgrad:tm192", "fwd:tm192", "dgrad:tm192"),
    xcase("n_64", (1131, 13824, 64), (None,), "fwd:n_lt_256", "fwd:n_mod256_64", placing="offset"),
    # the input gradient's N = I below one column tile; more than 1024 rows: the weight gradient in two slabs
    xcase("dgrad_n_240", (520, 240, 8208), (None,), "dgrad:n_lt_256", "dgrad:n_mod256_240", "wgrad:n_mod256", placing="exact"),
    # the XCD renumbering with fewer blocks than XCDs: one 192-row tile, one column tile, the input gradient's four splits
    xcase("few_blocks", (192, 256, 20352), (192,), "dgrad:blocks_lt_8", "dgrad:tm192", "dgrad:splits_2_8"),
    # every tile height in every role, one row into a new tile of each; O and I no multiples of the tile
    xcase("tile_heights", (385, 1648, 1584), (64, 128, 192, 256), "fwd:m_mod_tm_1", "dgrad:m_mod_tm_1", "fwd:tm64", "fwd:tm128",
          "fwd:tm192", "dgrad:tm64", "dgrad:tm128", "dgrad:tm192", "wgrad:tm64", "wgrad:tm128", "wgrad:tm192", "wgrad:tm256",
          "wgrad:m_mod_tm", "wgrad:n_mod256"),
]

_GX_FD = ("tm64", "tm128", "tm192", "splits_1", "splits_2_8", "last_split_short", "n_mod256_16", "n_mod256_240", "n_lt_256",
          "m_lt_tm", "m_mod_tm_1", "fold")
GX_REQUIRED = ({"fwd:" + l for l in _GX_FD} | {"dgrad:" + l for l in _GX_FD} | {"fwd:splits_gt_8"} |
               {"wgrad:" + l for l in ("tm64", "tm128", "tm192", "tm256", "rp_32", "rp_15_zero_rows", "m_mod_tm", "n_mod256",
                                       "steps_lt_ring", "splits_1", "splits_2_8", "last_split_short", "fold")} |
               {"%s:%s" % (f, l) for f in FORMS.values() for l in ("blocks_mod8", "blocks_lt_8", "fwd", "dgrad", "wgrad")} |
               {"f16x3:steps_lt_ring"})


def gx_runs(cases=None):
    """every test of the gemmx part: (case, forced tile height, input range); a run issues all three roles in both forms"""
    runs = []
    for c in (GX_CASES if cases is None else cases):
        for tm in c["tms"]:
            runs.append(dict(name=c["name"], shape=c["shape"], tm=tm, placing=c["placing"], wide=False))
        if c["wide"]:
            runs.append(dict(name=c["name"], shape=c["shape"], tm=None, placing=c["placing"], wide=True))
    return runs


def gx_launches_of_run(r):
    return [gx_launch(role, r["shape"], form, r["tm"]) for role in ROLES for form in FORMS]


def gx_labels_of_run(r):
    L = set()
    for p in gx_launches_of_run(r):
        L |= gx_labels(p)
    if r["wide"]:
        L.add("wide_range")
    return L


GX_REQUIRED |= {"wide_range"}
REQUIRED = F32_REQUIRED | GX_REQUIRED


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def linear_inputs(rng, shape, wide=False):
    """-> x, w, b, gy, gw0, gb0 (fp32) of one run.  x and gy as tests/test_gpu_elem.py draws the large Linear's (x with a few
    decades of range downwards, gy / R); wide: every element of the two activation operands scaled by 2^0 .. 2^-11 instead:
    twelve binades.  gw0, what the weight gradient is added to, is of the size of that product."""
    import numpy as np
    R, I, O = shape
    x = rng.randn(R, I).astype(np.float32)
    gy = (rng.randn(R, O) / R).astype(np.float32)
    if wide:
        x = (x * np.exp2(-rng.randint(0, 12, size=x.shape))).astype(np.float32)
        gy = (gy * np.exp2(-rng.randint(0, 12, size=gy.shape))).astype(np.float32)
    else:
        x[:, ::7] *= 1e-3
        x[min(3, R - 1)] *= 1e-2
    w = (rng.randn(O, I) / np.sqrt(I)).astype(np.float32)
    b = rng.randn(O).astype(np.float32)
    gw0 = (rng.randn(O, I) / np.sqrt(R)).astype(np.float32)
    gb0 = rng.randn(O).astype(np.float32)
    return x, w, b, gy, gw0, gb0


def find(name):
    for c in F32_CASES + GX_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)
