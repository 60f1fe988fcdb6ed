"""Staged training on the host (no device): cfg["train"] validation, the trainable ranges of a parameter layout, the complement
logic the optimisers and the data-parallel exchange use, and the C ABI's new entry points in the Lua binding."""
import os
import re

import pytest

import frcnn_amd as F
from frcnn_amd import objective as OBJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a hand-made layout: four blocks, the anchor nets, the classification net
BLOCKS = [(0, 100), (100, 250), (250, 600), (600, 1000)]
HEADS = (1000, 1100)
CNET = (1100, 3000)


@pytest.mark.parametrize("train, want", [
    (None, (0, True, True)),
    ({}, (0, True, True)),
    (dict(proposal=True, classification=False), (0, True, False)),
    (dict(proposal=False, classification=True, frozen_blocks=4), (4, False, True)),
    (dict(frozen_blocks=2), (2, True, True)),
])
def test_settings(train, want):
    cfg = {} if train is None else dict(train=train)
    assert OBJ.train_settings(cfg, 4) == want


@pytest.mark.parametrize("train", [
    dict(proposal=False, classification=False),
    dict(frozen_blocks=5), dict(frozen_blocks=-1), dict(frozen_blocks=1.5), dict(frozen_blocks=True),
    dict(proposal=1), dict(classification="yes"), dict(freeze=2), "all",
])
def test_bad_settings_raise(train):
    with pytest.raises(F.FrcnnError):
        OBJ.train_settings(dict(train=train), 4)


@pytest.mark.parametrize("fb, prop, clsf, want", [
    (0, True, True, [(0, 3000)]),
    (0, True, False, [(0, 1100)]),
    (0, False, True, [(0, 1000), (1100, 3000)]),
    (4, True, False, [(1000, 1100)]),
    (4, False, True, [(1100, 3000)]),
    (2, True, True, [(250, 3000)]),
    (3, False, True, [(600, 1000), (1100, 3000)]),
])
def test_trainable_ranges(fb, prop, clsf, want):
    assert OBJ.trainable_ranges(BLOCKS, HEADS, CNET, fb, prop, clsf) == want


def test_nothing_trainable_raises():
    with pytest.raises(F.FrcnnError):
        OBJ.trainable_ranges(BLOCKS, HEADS, (3000, 3000), 4, False, True)


def test_uncovered_is_the_complement_within_the_ranges():
    # the whole vector: the gaps between the slices already handled (what _step / allreduce_begin_rest always computed)
    assert OBJ.uncovered([(1100, 3000), (1000, 1100), (600, 1000), (250, 600)], [(0, 3000)]) == [(0, 250)]
    assert OBJ.uncovered([], [(0, 3000)]) == [(0, 3000)]
    assert OBJ.uncovered([(0, 3000)], [(0, 3000)]) == []
    assert OBJ.uncovered([(5, 5), (10, 20)], [(0, 30)]) == [(0, 5), (5, 10), (20, 30)]
    # staged: only what is trainable and not done yet
    assert OBJ.uncovered([(1100, 3000)], [(600, 1000), (1100, 3000)]) == [(600, 1000)]
    assert OBJ.uncovered([(700, 800)], [(600, 1000), (1100, 3000)]) == [(600, 700), (800, 1000), (1100, 3000)]
    assert OBJ.uncovered([(1000, 1100)], [(1000, 1100)]) == []


def test_lua_binding_declares_the_new_entry_points():
    txt = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    for name in ("frcnn_model_set_trainable", "frcnn_model_get_trainable", "frcnn_nag_lookahead_slice"):
        assert re.search(r"\bint %s\(" % name, txt), name
        assert name in F._lib.exported_symbols()
