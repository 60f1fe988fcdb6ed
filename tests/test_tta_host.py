"""Test-time augmentation without a GPU: the setting's validation (tta_settings, Detector.set_tta, Detector(model, tta=...)),
the view list (order, sizes, truncation), the call-time refusals, the identity table, hand-worked cases of the restatement
(tests/tta_ref.py), and static checks of the surfaces (ctypes row, export, generated cdef, Lua drop-in)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tta_ref as T
from test_abi import ROOT, _lua_code


class _Untouchable(object):
    """stands for the model (or a frame's data): any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("touched (%s) before the setting was checked" % name)

    def __getitem__(self, key):
        raise AssertionError("touched ([%r]) before the setting was checked" % (key,))


class _CfgOnly(dict):
    """a model of which only the cfg may be read"""

    def __getitem__(self, key):
        if key != "cfg":
            raise AssertionError("the model was touched ([%r]) before the setting was checked" % (key,))
        return dict.__getitem__(self, key)


def _settings():
    from frcnn_amd.Detector import tta_settings
    return tta_settings


# ------------------------------------------------------------------------------------------------ the setting
def test_tta_settings_defaults_and_accepted_tables():
    ts = _settings()
    assert ts(None) is None and ts(dict(class_count=16)) is None and ts(dict(class_count=16, tta=None)) is None
    assert ts({}) == (False, (1.0,)) == ts(dict(class_count=16, tta={}))
    assert ts(dict(hflip=True)) == (True, (1.0,))
    assert ts(dict(scales=[1, 1.25])) == (False, (1.0, 1.25))
    assert ts(dict(scales=(0.5, np.float32(2.0), np.int64(1)), hflip=np.bool_(True))) == (True, (0.5, 2.0, 1.0))
    assert ts(dict(class_count=16, tta=dict(hflip=False, scales=[1.5]))) == (False, (1.5,))


@pytest.mark.parametrize("table", [
    dict(flip=True), dict(hflip=True, vflip=True), dict(scale=[1.0]),
    dict(hflip=1), dict(hflip=0), dict(hflip="true"), dict(hflip=None), dict(hflip=[True]),
    dict(scales=[]), dict(scales=()), dict(scales=1.0), dict(scales=None), dict(scales="1.0"), dict(scales={1.0: 1}),
    dict(scales=np.array([1.0, 1.25])),
    dict(scales=[True]), dict(scales=[1.0, False]), dict(scales=["1.0"]), dict(scales=[None]), dict(scales=[[1.0]]),
    dict(scales=[float("nan")]), dict(scales=[float("inf")]), dict(scales=[0]), dict(scales=[0.0]), dict(scales=[-1.0]), dict(scales=[1.0, -0.5]),
    dict(scales=[1.0, 1.0]), dict(scales=[1, 1.0]), dict(scales=[1.25, 1.0, 1.25]),
    "hflip", 1.0, [1.0], True,
])
def test_tta_settings_rejects(table):
    with pytest.raises(ValueError):
        _settings()(table)
    if isinstance(table, dict):
        with pytest.raises(ValueError):
            _settings()(dict(class_count=16, tta=table))


def test_detector_refuses_a_bad_table_before_the_model_or_the_device_is_touched():
    import inspect
    import frcnn_amd as F
    from frcnn_amd.Detector import Detector
    for bad in (dict(flip=True), dict(hflip=1), dict(scales=[]), dict(scales=1.0), dict(scales=[True]), dict(scales=["a"]),
                dict(scales=[float("nan")]), dict(scales=[0.0]), dict(scales=[2.0, 2.0]), "hflip"):
        with pytest.raises(ValueError):
            Detector(_Untouchable(), tta=bad)                    # refused before the model is looked at
        with pytest.raises(ValueError):
            Detector(_Untouchable(), static_weights=True, tta=bad)
        if isinstance(bad, dict):
            with pytest.raises(ValueError):
                Detector(_CfgOnly(cfg=dict(F.duplo_cfg, tta=bad)))   # main.lua's Detector(model): the cfg carries it
    assert list(inspect.signature(Detector.__init__).parameters)[1:] == ["model", "static_weights", "proposals", "nms"]
    assert Detector.tta_settings(dict(hflip=True)) == (True, (1.0,))
    d = Detector.__new__(Detector)
    d.set_tta(dict(class_count=16))
    assert d.tta is None
    d.set_tta(dict(class_count=16, tta=dict(scales=[1, 2])))
    assert d.tta == (False, (1.0, 2.0))
    with pytest.raises(ValueError):
        d.set_tta(dict(scales=[1, 1]))
    assert d.tta == (False, (1.0, 2.0)), "a refused table changes nothing"
    d.set_tta(None)
    assert d.tta is None


# ------------------------------------------------------------------------------------------------ the views
def test_view_order_and_sizes():
    from frcnn_amd.Detector import tta_views
    H, W = 128, 176
    assert tta_views(None, H, W) == [(1.0, False, H, W)] == tta_views((False, (1.0,)), H, W)
    assert tta_views((True, (1.0,)), H, W) == [(1.0, False, H, W), (1.0, True, H, W)]
    # scale-major in the order given, the unmirrored view first
    got = tta_views((True, (1.25, 1.0, 0.5)), H, W)
    assert got == [(1.25, False, 160, 220), (1.25, True, 160, 220), (1.0, False, H, W), (1.0, True, H, W), (0.5, False, 64, 88),
                   (0.5, True, 64, 88)]
    # truncation (BatchIterator.lua:52), not rounding: 128 * 1.3 = 166.4, 176 * 1.3 = 228.8; and a product just under an integer:
    # 1.15 * 100 is 114.99999999999999 in fp64 -> 114
    assert tta_views((False, (1.3,)), H, W) == [(1.3, False, 166, 228)]
    assert 1.15 * 100 < 115 and tta_views((False, (1.15,)), 100, 100) == [(1.15, False, 114, 114)]
    assert tta_views((False, (0.001,)), H, W) == [(0.001, False, 1, 1)], "at least one pixel"
    for settings in (None, (False, (1.0,)), (True, (1.0,)), (True, (1.25, 1.0, 0.5)), (False, (1.3, 0.7))):
        hflip, scales = settings or (False, (1.0,))
        for h, w in ((H, W), (130, 131)):
            assert tta_views(settings, h, w) == T.views(hflip, scales, h, w)


class _FakeDetector(object):
    """Detector without a model: the host arithmetic of a frame's layout from fixed layer lists"""

    def __new__(cls, tta, batch=8):
        from frcnn_amd.Detector import Detector, _Layout

        def layout_of(self, H, W):     # four head maps that shrink by 16 and lose a border of 2
            hw = [(H // 16 - 2 - i, W // 16 - 2 - i) for i in range(4)]
            return _Layout(hw, (8, H // 16, W // 16), [0] * 5, 0, 0)
        D = type("D", (Detector,), dict(_layout_of=layout_of))
        d = D.__new__(D)
        d.set_tta(tta)
        d.BATCH = batch
        return d


def test_call_time_refusals_come_before_anything_is_queued():
    frame = (3, 128, 176)
    assert _FakeDetector(dict(hflip=True, scales=[1, 1.25, 1.5, 2]))._view_lists([frame])[0][-1] == (2.0, True, 256, 352)   # V = 8
    with pytest.raises(ValueError) as e:
        _FakeDetector(dict(hflip=True, scales=[1, 1.25, 1.5, 2, 3]))._view_lists([frame])
    assert "10 views" in str(e.value)
    with pytest.raises(ValueError):
        _FakeDetector(dict(hflip=True), batch=1)._view_lists([frame])
    assert len(_FakeDetector(dict(hflip=True), batch=2)._view_lists([frame, frame])) == 2
    # 128 x 176 at 0.5: 64 x 88 -> head maps (2, 3), (1, 2), (0, 1): empty
    with pytest.raises(ValueError) as e:
        _FakeDetector(dict(scales=[1, 0.5]))._view_lists([frame])
    assert "0.5" in str(e.value)
    _FakeDetector(dict(scales=[1, 0.5]))._view_lists([(3, 256, 352)])
    # detect() and detect_batch() ask before they look at a frame's data or the model (the Detector has neither)
    from frcnn_amd.tensor import DeviceTensor
    ghost = DeviceTensor(0, frame)
    for tta in (dict(hflip=True, scales=[1, 1.25, 1.5, 2, 3]), dict(scales=[1, 0.5])):
        d = _FakeDetector(tta)
        with pytest.raises(ValueError):
            d.detect(ghost)
        with pytest.raises(ValueError):
            d.detect_batch([ghost, ghost])


def test_an_identity_table_is_off():
    for tta in (None, {}, dict(hflip=False), dict(scales=[1]), dict(scales=[1.0], hflip=False)):
        d = _FakeDetector(tta)
        assert d._view_lists([(3, 128, 176)]) is None, tta
    assert _FakeDetector(dict(hflip=True))._view_lists([(3, 128, 176)]) == [[(1.0, False, 128, 176), (1.0, True, 128, 176)]]
    assert _FakeDetector(dict(scales=[1.25]))._view_lists([(3, 128, 176)]) == [[(1.25, False, 160, 220)]]   # one view, not the frame


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_to_frame_by_hand():
    r = np.array([[0.0, 2.0, 10.0, 8.0], [30.0, 1.0, 100.0, 5.0]])
    assert T.to_frame(r, 0, 100.0, 1.0, 1.0).tobytes() == r.tobytes()
    assert T.to_frame(r, 1, 100.0, 1.0, 1.0).tolist() == [[90.0, 2.0, 100.0, 8.0], [0.0, 1.0, 70.0, 5.0]]
    assert T.to_frame(r, 0, 100.0, 0.5, 2.0).tolist() == [[0.0, 4.0, 5.0, 16.0], [15.0, 2.0, 50.0, 10.0]]
    assert T.to_frame(r, 1, 100.0, 0.5, 2.0).tolist() == [[45.0, 4.0, 50.0, 16.0], [0.0, 2.0, 35.0, 10.0]]
    # un-mirroring is its own inverse
    assert T.to_frame(T.to_frame(r, 1, 100.0, 1.0, 1.0), 1, 100.0, 1.0, 1.0).tobytes() == r.tobytes()
    # the factors of a view are frame / view: 176 / 220 = 0.8 exactly, 128 / 166 is not
    g = T.geometry(T.views(True, [1.0, 1.3], 128, 176), 128, 176)
    assert g[0] == (0, 176.0, 1.0, 1.0) and g[1] == (1, 176.0, 1.0, 1.0) and g[3] == (1, 228.0, 176.0 / 228, 128.0 / 166)


def test_merge_by_hand():
    v0 = dict(bb=np.array([[1, 2, 3, 4, -0.5]], np.float32), kc=[3], keep_row=[1], r2=[[1, 2, 3, 4]], pick=[5, 2], n=7)
    v1 = dict(bb=np.zeros((0, 5), np.float32), kc=[], keep_row=[], r2=np.zeros((0, 4)), pick=[], n=0)
    v2 = dict(bb=np.array([[0, 0, 0, 0, -0.25], [0, 0, 0, 0, -0.125]], np.float32), kc=[3, 9], keep_row=[0, 2],
              r2=[[10, 2, 30, 4], [0, 0, 100, 8]], pick=[1, 9, 4], n=9)
    m = T.merge([v0, v1, v2], [(0, 100.0, 1.0, 1.0), (1, 100.0, 1.0, 1.0), (1, 100.0, 2.0, 0.5)], 20)
    assert m["roff"].tolist() == [0, 2, 2, 5] and m["counts"] == (16, 5, 3)
    assert m["pick"].tolist() == [5, 2, 41, 49, 44] and m["keep_row"].tolist() == [1, 2, 4] and m["kc"].tolist() == [3, 3, 9]
    assert m["r2"].tolist() == [[1, 2, 3, 4], [140, 1, 180, 2], [0, 0, 200, 4]]
    assert m["bb"].tolist() == [[1, 2, 3, 4, -0.5], [140, 1, 180, 2, -0.25], [0, 0, 200, 4, -0.125]]
    assert [T.view_of(c, m["roff"]) for c in (1, 2, 3, 5)] == [0, 0, 2, 2]


# ------------------------------------------------------------------------------------------------ the surfaces
def test_surfaces_name_the_entry_point():
    import frcnn_amd as F
    assert "frcnn_detect_merge_views" in F._lib.exported_symbols()
    assert len(F._lib._SIGS["frcnn_detect_merge_views"][0]) == 22
    assert not [n for n in F._lib.KC_NAMES if "tta" in n or "merge" in n or "view" in n], "counted under elemwise: no new kernel class"
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_lua_binding.py"), "--check"]) == 0, \
        "bindings/frcnn_hip.lua is stale: run python tools/gen_lua_binding.py"
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert "int frcnn_detect_merge_views(const float *bb, const int *kc, const int *keep_row, const double *r2" in cdef
    det = _lua_code(open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read())
    assert "function Detector.tta_settings" in det and "function Detector:set_tta" in det and "cfg.tta" in det and "opts.tta" in det
    assert "C.frcnn_image_scale(" in det and "C.frcnn_image_crop_flip(" in det
    # the drop-in merges between the class test and the per-class pass, and the gather comes last
    a, b, c, e = (det.index(t) for t in ("C.frcnn_detect_post(", "C.frcnn_detect_merge_views(", "C.frcnn_nms_device_batch(dbb",
                                         "C.frcnn_detect_gather_batch("))
    assert a < b < c < e
    src = open(os.path.join(ROOT, "faster-rcnn.torch_amd", "csrc", "detect.hip")).read()
    assert "detect_merge_views_kernel" in src and "KC_ELEMWISE" in src[src.index("int detect_merge_views("):]
