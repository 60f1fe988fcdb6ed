"""The tables of tests/test_gpu_nms_scan.py have the closed-form answers they claim (against the CPU oracle) and reach every
wave role of the greedy scan they exist for (tests/nms_plan.py restates the roles; no GPU needed).  A retune of the scan's
constants or a later edit of the tables cannot drop a role without this failing."""
import os
import re

import numpy as np
import pytest

import nms_plan as NP
from util import random_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernel_file_s():
    text = open(os.path.join(ROOT, "faster-rcnn.torch_amd", "csrc", "nms.hip")).read()

    def define(name):
        found = re.findall(r"^#define\s+%s\s+(\S+)" % name, text, re.M)
        assert len(found) == 1, (name, found)
        return found[0]
    assert int(define("NMS_LEAD")) == NP.LEAD
    assert int(define("NMS_BG_ITEMS")) == NP.BG_ITEMS
    assert int(define("NMS_RED_THREADS")) == NP.RED_THREADS
    assert int(define("NMS_RANK_SLICE")) == NP.RANK_SLICE
    assert define("NMS_NU") == "NMS_LEAD" and NP.NU == NP.LEAD
    assert "#define NMS_BG_WAVES (NMS_RED_THREADS / 64 - 2 - NMS_NU)" in text
    assert NP.BG_WAVES == 10


@pytest.fixture(scope="module")
def analysed():
    """the restated greedy pass over every table entry, once"""
    return {p["name"]: NP.analyse(p["rows"], p["thr"]) for p in NP.ALL}


def test_the_oracle_gives_the_closed_forms(O, analysed):
    assert len({p["name"] for p in NP.ALL}) == len(NP.ALL)
    for p in NP.ALL:
        assert O.nms(p["rows"], p["thr"]).tolist() == p["expect"], p["name"]
        assert analysed[p["name"]]["pick"] == p["expect"], p["name"]      # the restatement that labels agrees
    assert NP.DEGENERATE["expect"] == [4, 3]
    # what the closed forms amount to
    s = NP.SCAN_CASE
    assert s["n"] == 4603 and len(s["pairs"]) == 146 and len(s["expect"]) == 4603 - 146 - 75
    assert s["row_of"][s["n"] - 1] + 1 not in s["expect"]                  # the very last position is a victim
    assert len(NP.ALL_KEPT["expect"]) == 1000 and len(NP.ONE_KEPT["expect"]) == 1
    assert NP.CHAIN_ALONE["expect"] == [int(NP.CHAIN_ALONE["row_of"][j]) + 1 for j in range(0, 150, 2)]
    assert NP.EQUAL_KEYS["expect"] == [r for r in range(700, 0, -1) if r not in (6, 300)]
    assert [p["n"] for p in NP.EDGE_SIZES] == [64 * k + e for k in range(1, 8) for e in (-1, 0, 1)]
    for p in NP.EDGE_SIZES:
        assert len(p["expect"]) == p["n"] - 2 and p["pairs"][0] == (0, p["n"] - 1)
        assert sorted(p["row_of"].tolist()) == list(range(p["n"])) and p["row_of"].tolist() != list(range(p["n"]))


def test_the_oracle_gives_the_class_aware_closed_form(O):
    s = NP.SCAN_CASE
    cls, expect = NP.with_classes(s)
    rows = s["rows"]
    crossed = [q for k, (p, q) in enumerate(s["pairs"]) if k % 2]
    assert len(expect) == len(s["expect"]) + len(crossed) == len(s["expect"]) + 73
    row_cls = lambda pos: int(cls[s["row_of"][pos]])
    for k, (p, q) in enumerate(s["pairs"]):
        assert (row_cls(p) != row_cls(q)) == bool(k % 2)
    ids = []
    for c in np.unique(cls):                  # one nms per class, merged back into global pick order (the keys are unique)
        r = np.nonzero(cls == c)[0]
        ids += [int(r[i - 1]) + 1 for i in O.nms(rows[r], s["thr"]).tolist()]
    assert sorted(ids, key=lambda i: -rows[i - 1, 3]) == expect


def test_tables_reach_every_role(analysed):
    """Coverage from the pick lists, not from the construction: a suppressed box counts for a role only if every kept row that
    suppresses it acts through that role -- only then would a fault in the role change the answer."""
    scan = analysed["scan"]["sole"]
    missing = sorted(set(NP.LABELS) - set(scan))
    assert not missing, missing
    print("SCAN_CASE, boxes decided by one role alone:", scan)
    labels = set()
    for p in NP.ALL:
        labels |= NP.labels_of(p)
    assert NP.REQUIRED <= labels, sorted(NP.REQUIRED - labels)
    assert "chain_full_group" in NP.labels_of(NP.CHAIN_ALONE) and "chain_full_group" in NP.labels_of(NP.SCAN_CASE)
    assert "equal_keys_across_rank_blocks" in NP.labels_of(NP.EQUAL_KEYS)
    assert NP.rank_blocks_of_equal_keys(NP.EQUAL_KEYS["rows"][:, 3]) == (3, True)
    assert analysed["all_kept"]["kept_max"] == 64 and analysed["all_kept"]["sole"] == {}
    assert analysed["scan"]["rounds_max"] == 64 and analysed["scan"]["kept_max"] == 64


def test_the_designed_ranks_and_distances_are_there():
    """role() at the corners of the design: ranks 0 / 9 / 10 / 19 in registers and 20 / 39 / 40 / 62 at once behind group 0 (two
    pieces), 39 / 40 on either side behind group 12 (one piece); word distances 5 / 6 (last helper / first background word)
    and 69 / 70 (last word of the first piece / first of the second)."""
    nw = NP.cdiv(NP.SCAN_N, 64)
    assert nw == 72 and NP.cdiv(nw - (0 + 2 + NP.NU), 64) == 2 and NP.cdiv(nw - (12 + 2 + NP.NU), 64) == 1
    word = lambda G, d: 64 * (G + d)
    assert [NP.role(r, r, word(0, 6), nw) for r in NP.SCAN_RANKS] == ["bg_reg_chunk0"] * 4 + ["bg_now_chunk0"] * 4
    assert [NP.role(r, r, word(0, 69), nw) for r in NP.SCAN_RANKS] == ["bg_reg_chunk0"] * 4 + ["bg_now_chunk0"] * 4
    assert [NP.role(r, r, word(0, 70), nw) for r in NP.SCAN_RANKS] == ["bg_reg_chunk1"] * 4 + ["bg_now_chunk1"] * 4
    assert [NP.role(r, r, word(0, 71), nw) for r in NP.SCAN_RANKS] == ["bg_reg_chunk1"] * 4 + ["bg_now_chunk1"] * 4
    assert [NP.role(64 * 12 + r, r, word(12, 7), nw) for r in NP.SCAN_RANKS] == ["bg_reg_chunk0"] * 6 + ["bg_now_chunk0"] * 2
    assert [NP.role(5, 5, word(0, d), nw) for d in range(7)] == ["diag", "next_word", "helper1", "helper2", "helper3", "helper4",
                                                                  "bg_reg_chunk0"]
    s = NP.SCAN_CASE
    victims = {}
    for p, q in s["pairs"]:
        victims.setdefault(p, []).append(q // 64 - p // 64)
    assert sorted(victims) == [64 * G + r for G in NP.SCAN_GROUPS for r in NP.SCAN_RANKS]
    for p, ds in victims.items():
        want = set(range(1, 8)) | ({69, 70, 71} if p < 64 else {59})
        assert want <= set(ds) <= want | {0}, (p, sorted(ds))
    assert {d for ds in victims.values() for d in ds} >= {0}
    for G in NP.SCAN_GROUPS:       # a suppressor's offset is its rank: no victim in front of it in its group
        assert [q for q in s["victims"] if q // 64 == G] == [64 * G + 63]


def test_a_scan_without_one_role_misses_the_closed_form():
    """the restated pass with one role's ORs left out: SCAN_CASE's pick list changes for every role behind the diagonal, while
    test_nms_matches_oracle's n = 2000 input does not notice the loss of the roles the tables were built for"""
    s = NP.SCAN_CASE
    for lab in NP.LABELS[1:]:
        assert NP.analyse(s["rows"], s["thr"], drop={lab})["pick"] != s["expect"], lab
    b = random_boxes(np.random.RandomState(2000), 2000)
    new = {"bg_reg_chunk1", "bg_now_chunk0", "bg_now_chunk1"}
    assert NP.analyse(b, 0.25, drop=new)["pick"] == NP.analyse(b, 0.25)["pick"]


def test_random_boxes_do_not_reach_the_new_roles():
    """Why the tables exist: the distribution every other NMS test draws from decides no box through the background waves'
    immediate loop or through a second 64-word piece (test_nms_matches_oracle's n = 6000, thr = 0.25), and its diagonal loop
    stays under half a group's depth."""
    b = random_boxes(np.random.RandomState(6000), 6000)
    a = NP.analyse(b, 0.25)
    print("random_boxes n = 6000, thr 0.25: kept %d, most kept in a group %d, most ballot rounds %d, sole %s"
          % (len(a["pick"]), a["kept_max"], a["rounds_max"], a["sole"]))
    assert not [l for l in a["sole"] if l.startswith("bg_now") or l.endswith("chunk1")], a["sole"]
    # the immediate loop starts at rank 40 with one piece behind the group; a chain through a whole group takes 64 rounds
    assert a["kept_max"] < 40 and a["rounds_max"] < 32
