"""The per-size layout of the Detector's front (Detector._layout, _chunk_slots) without a GPU: host arithmetic on plain layer
lists, checked against an independent restatement -- per layer ceil((n + 2p - k) / d) + 1 in floating point, ceil-64 prefix
offsets, 3 * sum(h * w) anchors -- for the layer lists of vgg_small and vgg_large at the sizes of tests/test_gpu_detect_mixed.py,
at 450x800 and at 600x1000, and against two sizes the repository states elsewhere."""
import math

import pytest

from util import VGG_SMALL_HEADS, VGG_SMALL_LAYERS

VGG_LARGE_LAYERS = [dict(filters=64, kW=3, padW=1, conv_steps=2), dict(filters=128, kW=3, padW=1, conv_steps=2),
                    dict(filters=256, kW=3, padW=1, conv_steps=3), dict(filters=512, kW=3, padW=1, conv_steps=3)]
MODELS = dict(vgg_small=(VGG_SMALL_LAYERS, VGG_SMALL_HEADS), vgg_large=(VGG_LARGE_LAYERS, VGG_SMALL_HEADS))   # (the same heads)
SIZES = [(128, 176), (128, 192), (144, 176), (176, 128), (450, 800), (600, 1000)]      # (H, W)


def _layer_lists(layers, heads):
    """rows (kW, kH, dW, dH, padW, padH) on the way to each of the five outputs, as the native model lists them: per block its
    convolutions (stride 1) and a 2x2 / stride-2 pooling; a head adds its k x k and its 1x1 convolution, unpadded"""
    def blocks(n):
        rows = []
        for l in layers[:n]:
            rows += [(l["kW"], l["kW"], 1, 1, l["padW"], l["padW"])] * l["conv_steps"] + [(2, 2, 2, 2, 0, 0)]
        return rows
    return [blocks(h["input"]) + [(h["kW"], h["kW"], 1, 1, 0, 0), (1, 1, 1, 1, 0, 0)] for h in heads] + [blocks(len(layers))]


def _restated(lists, planes, H, W):
    hw = []
    for rows in lists:
        h, w = H, W
        for kW, kH, dW, dH, pW, pH in rows:
            h, w = int(math.ceil((h + 2 * pH - kH) / float(dH))) + 1, int(math.ceil((w + 2 * pW - kW) / float(dW))) + 1
        hw.append((h, w))
    ceil64 = lambda n: int(math.ceil(n / 64.0)) * 64
    hoff = [0]
    for h, w in hw[:4]:
        hoff.append(hoff[-1] + ceil64(18 * h * w))
    fh, fw = hw[4]
    return dict(hw=hw[:4], fshape=(planes, fh, fw), hoff=hoff, fslot=ceil64(planes * fh * fw), anchors=3 * sum(h * w for h, w in hw[:4]))


def _layouts(name, sizes):
    from frcnn_amd.Detector import _layout
    layers, heads = MODELS[name]
    lists = _layer_lists(layers, heads)
    return [_layout(lists, layers[-1]["filters"], H, W) for H, W in sizes], lists, layers[-1]["filters"]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_layout_against_its_restatement(name):
    got, lists, planes = _layouts(name, SIZES)
    for (H, W), t in zip(SIZES, got):
        want = _restated(lists, planes, H, W)
        assert [tuple(m) for m in t.hw] == want["hw"] and tuple(t.fshape) == want["fshape"], (name, H, W)
        assert list(t.hoff) == want["hoff"] and len(t.hoff) == 5 and t.fslot == want["fslot"] and t.anchors == want["anchors"], (name, H, W)
        assert all(o % 64 == 0 for o in t.hoff) and t.fslot % 64 == 0 and t.fslot >= planes * t.fshape[1] * t.fshape[2]


def test_layout_at_sizes_stated_elsewhere():
    """vgg_small's head maps of a 450x800 frame (tests/test_gpu_detect_batch.py); vgg_large 600x1000 scans 45 015 anchors"""
    (small,), _, _ = _layouts("vgg_small", [(450, 800)])
    assert [tuple(m) for m in small.hw] == [(55, 98), (27, 48), (25, 46), (23, 44)] and small.fshape[0] == 384
    (large,), _, _ = _layouts("vgg_large", [(600, 1000)])
    assert large.anchors == 45015 and large.fshape[0] == 512


@pytest.mark.parametrize("name", sorted(MODELS))
def test_chunk_strides_are_those_of_the_largest_frame(name):
    from frcnn_amd.Detector import _chunk_slots
    lay, _, _ = _layouts(name, SIZES)
    chunks = [lay[:4], [lay[0], lay[2], lay[3]], lay[4:], lay]
    for chunk in chunks:
        assert _chunk_slots(chunk) == (max(t.hoff[4] for t in chunk), max(t.fslot for t in chunk), max(t.anchors for t in chunk))
    slot, fslot, cap = _chunk_slots(lay[:4])
    assert all(t.hoff[4] <= slot and t.fslot <= fslot and t.anchors <= cap for t in lay[:4])
    assert len(set(t.hoff[4] for t in lay[:4])) > 1, "the mixed test sizes need slots of different sizes"
    for t in lay:     # a chunk of one size: the slot is the frame's own extent, as the one-size front had it
        assert _chunk_slots([t] * 3) == (t.hoff[4], t.fslot, t.anchors) == _chunk_slots([t])
