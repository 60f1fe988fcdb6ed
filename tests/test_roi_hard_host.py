"""Online hard example mining (cfg.roi_sampling.source = "hard") without a GPU: the setting is accepted and refused as documented,
the numpy restatement the device tests compare against (tests/roi_hard_ref.py) has the properties that define the selection, and
the two entry points are declared for the Lua host."""
import math
import os
import re

import numpy as np
import pytest

import roi_hard_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hard_is_a_source_and_hard_nms_overlap_a_key(F):
    from frcnn_amd.objective import ROI_SAMPLING_DEFAULTS
    assert ROI_SAMPLING_DEFAULTS["hard_nms_overlap"] == 0.7 and ROI_SAMPLING_DEFAULTS["source"] == "examples"
    rs = F.roi_sampling_settings(dict(roi_sampling=dict(source="hard")))
    assert rs["source"] == "hard" and rs["hard_nms_overlap"] == 0.7 and rs["batch"] == 128
    assert F.roi_sampling_settings(dict(roi_sampling=dict(source="hard", hard_nms_overlap=1)))["hard_nms_overlap"] == 1.0
    assert F.roi_sampling_settings(dict(roi_sampling=dict(source="hard", hard_nms_overlap=0.25, batch=16)))["hard_nms_overlap"] == 0.25
    # accepted and unused under the other sources, with their defaults unchanged
    for source in ("examples", "proposals"):
        rs = F.roi_sampling_settings(dict(roi_sampling=dict(source=source, hard_nms_overlap=0.3)))
        assert rs["source"] == source and rs["hard_nms_overlap"] == 0.3 and rs["fg_quota"] == 32
    # ... whose validated table is the one it was while the key is not given
    assert "hard_nms_overlap" not in F.roi_sampling_settings(dict(roi_sampling={}))
    assert "hard_nms_overlap" not in F.roi_sampling_settings(dict(roi_sampling=dict(source="proposals")))
    assert F.roi_sampling_settings({}) is None


@pytest.mark.parametrize("value", [0, 0.0, 1.5, -0.1, float("nan"), float("inf"), True, False, "0.7", None, (0.7,)],
                         ids=lambda v: "v_%r" % (v,))
def test_hard_nms_overlap_out_of_range_is_refused(F, value):
    with pytest.raises(F.FrcnnError, match="hard_nms_overlap"):
        F.roi_sampling_settings(dict(roi_sampling=dict(source="hard", hard_nms_overlap=value)))


def test_unknown_key_and_source_are_refused(F):
    with pytest.raises(F.FrcnnError, match="unknown key"):
        F.roi_sampling_settings(dict(roi_sampling=dict(source="hard", hard_overlap=0.5)))
    with pytest.raises(F.FrcnnError, match="source"):
        F.roi_sampling_settings(dict(roi_sampling=dict(source="hardest")))
    with pytest.raises(F.FrcnnError, match="batch"):
        F.roi_sampling_settings(dict(roi_sampling=dict(source="hard", batch=0)))


def test_keys_ref_is_the_loss_of_the_rows():
    """against a float64 evaluation: each row within the fp32 roundings of its own operations; the special values as documented"""
    rng = np.random.RandomState(11)
    c = H.edge_rows(H.random_table(rng, 200, 60, 17))
    box5, loss = H.keys_ref(c["roi"], c["crout"], c["crtarget"], c["ccout"], c["cctarget"], c["nfg"])
    assert box5.dtype == np.float32 and box5[:, :4].tobytes() == c["roi"].astype(np.float32).tobytes()
    assert box5[:, 4].tobytes() == loss.tobytes() and not np.any(np.isnan(loss))
    seen = dict(neg_inf=0, pos_inf=0, linear=0, quadratic=0)
    for r in range(200):
        t = c["cctarget"][r]
        if not (1 <= t <= 17):
            assert loss[r] == -np.inf
            seen["neg_inf"] += 1
            continue
        z = (c["crout"][r] - c["crtarget"][r]).astype(np.float32).astype(np.float64) if r < 60 else np.zeros(4)
        with np.errstate(all="ignore"):
            terms = np.where(np.abs(z) < 1, 0.5 * z * z, np.abs(z) - 0.5)
            exact = -float(c["ccout"][r, int(t) - 1]) + (10.0 * terms.sum() if r < 60 else 0.0)
        seen["linear"] += int(np.sum(np.abs(z) >= 1)); seen["quadratic"] += int(np.sum(np.abs(z) < 1))
        if math.isnan(exact):
            assert loss[r] == np.inf
            seen["pos_inf"] += 1
        elif math.isinf(exact):
            assert loss[r] == exact
        else:   # 2 roundings a term, 3 sums, the factor, the final sum: < 8 units of 2^-24 of the magnitudes added
            mag = abs(float(c["ccout"][r, int(t) - 1])) + 10.0 * np.abs(terms).sum()
            assert abs(float(loss[r]) - exact) <= 8 * 2.0 ** -24 * mag
    assert seen["neg_inf"] >= 4 and seen["pos_inf"] >= 2 and seen["linear"] > 20 and seen["quadratic"] > 20
    # |z| exactly 1 takes the linear branch: 1 - 0.5
    one = H.keys_ref(np.zeros((1, 4)), [[1, -1, 0, 0]], np.zeros((1, 4)), [[0.0, -1.0]], [1.0], 1)[1]
    assert one[0] == np.float32(10.0)


@pytest.mark.parametrize("seed", range(6))
def test_select_ref_properties(seed):
    rng = np.random.RandomState(100 + seed)
    n = int(rng.randint(40, 160)); nfg = int(rng.randint(0, n // 3)); batch = int(rng.choice([1, 8, 32, n]))
    overlap = float(rng.choice([0.3, 0.5, 0.7]))
    c = H.random_table(rng, n, nfg, 5, span=120.0, dup=0.1, equal_loss=0.15)
    box5, loss = H.keys_ref(c["roi"], c["crout"], c["crtarget"], c["ccout"], c["cctarget"], nfg)
    out = H.select_ref(box5, loss, nfg, batch, overlap, H.table_of(c))
    rows, pick = out["rows"], [int(p) - 1 for p in out["pick"]]
    F_, Bq, count, n_ = out["counts"]
    assert (count, n_) == (len(pick), n) and F_ + Bq == len(rows) == min(batch, count)
    # the order: ascending rows, that is foreground first, each in candidate order; src travels with its row
    assert rows == sorted(rows) and all(i < nfg for i in rows[:F_]) and all(i >= nfg for i in rows[F_:])
    assert out["src"].tolist() == c["src"][rows].tolist() and np.all(np.diff(out["src"]) > 0)
    assert out["loss"].tobytes() == loss[rows].tobytes() and out["roi"].tobytes() == c["roi"][rows].tobytes()
    # the picks: descending loss, equal losses by the higher row, no survivor overlaps an earlier one above the threshold
    for a, b in zip(pick, pick[1:]):
        assert loss[a] > loss[b] or (loss[a] == loss[b] and a > b)
    assert set(rows) == set(pick[:batch])
    lowest = min(loss[i] for i in rows)
    order = dict((p, k) for k, p in enumerate(pick))
    for i in range(n):
        if i in set(rows):
            continue
        if i in order:                                          # a survivor that was cut by `batch`
            assert order[i] >= batch and loss[i] <= lowest
        else:                                                   # suppressed by an earlier pick above the overlap
            assert any(not (H.iou_f32(box5, p, i) <= np.float32(overlap)) and (loss[p] > loss[i] or (loss[p] == loss[i] and p > i))
                       for p in pick)


@pytest.mark.parametrize("n,nfg", [(1, 0), (1, 1), (70, 20), (130, 0)])
def test_overlap_one_and_a_batch_of_n_select_every_row(n, nfg):
    c = H.random_table(np.random.RandomState(n), n, nfg, 3, span=60.0, dup=0.3, equal_loss=0.3)
    box5, loss = H.keys_ref(c["roi"], c["crout"], c["crtarget"], c["ccout"], c["cctarget"], nfg)
    out = H.select_ref(box5, loss, nfg, n, 1.0, H.table_of(c))
    assert out["rows"] == list(range(n)) and out["counts"] == (nfg, n - nfg, n, n)
    assert H.select_ref(box5, loss, nfg, 4096, 1.0, H.table_of(c))["rows"] == list(range(n))


def test_gather_ref_skips_picks_outside_the_segment():
    c = H.random_table(np.random.RandomState(2), 10, 4, 3)
    loss = np.arange(10, dtype=np.float32)
    out = H.gather_ref([0, 9, 11, 2, 5, 1], 6, 3, 10, 4, H.table_of(c), loss)
    assert out["rows"] == [1, 4, 8] and out["counts"] == (1, 2, 6, 10)
    assert H.gather_ref([3, 4], 0, 3, 10, 4, H.table_of(c), loss)["counts"] == (0, 0, 0, 10)


def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_are_declared_for_both_hosts(F):
    """The two entry points live in include/frcnn_hip_hard.h, which frcnn_hip.h includes.  What tests/test_abi.py checks for
    frcnn_hip.h is checked here for that header: the library exports what it declares, the host mirror's second ctypes table
    and the Lua binding's second generated cdef declare exactly that, and the Lua files call nothing else through their handle."""
    import ctypes
    names = {"frcnn_roi_hard_keys_batch", "frcnn_roi_hard_gather_batch"}
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_hard.h")).read()
    assert '#include "frcnn_hip_hard.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names == set(F._lib.HARD_SIGS) and not names & set(F._lib.exported_symbols())
    for name in names:
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m and len(m.group(1).split(",")) == len(F._lib.HARD_SIGS[name][0]), name
    lib = ctypes.CDLL(F._lib.SO_PATH)
    assert all(hasattr(lib, n) for n in names) and all(getattr(F._lib.load(), n).argtypes for n in names)
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    first = lua.index("]]")
    second = lua[lua.index("ffi.cdef[[", first):lua.index("]]", first + 2)]
    assert _symbols(second) == names
    used = set()
    for fn in ("frcnn_hip.lua", "objective_hip.lua", "Detector_hip.lua", "frcnn_shims.lua.in"):
        used |= set(re.findall(r"\bCH\.(frcnn_[a-z0-9_]+)", open(os.path.join(ROOT, "bindings", fn)).read()))
    assert used == names
    assert "roi_hard_select" in F.__all__ and callable(F.roi_hard_select)
    # the NMS between the two kernels is the library's own, and the header says that its arithmetic defines the setting
    text = hdr[hdr.index("Online hard example mining"):hdr.index("int frcnn_roi_hard_keys_batch(")]
    for word in ("frcnn_nms_device_batch", "+ 1", "HIGHER row", "ASCENDING ROW ORDER"):
        assert word in text, word
