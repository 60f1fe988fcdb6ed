"""The life of a native model's events, streams and buffers (csrc/own.h, csrc/net.cpp): a re-shape that re-allocates the ring
of per-step tables of the compact blocks, models created, used and destroyed in a row, and the entry points that wait for
events nobody has recorded yet."""
import ctypes as C
import gc

import numpy as np
import pytest

import width_plan as WP

pytestmark = pytest.mark.gpu

# The narrowest backbone of tests/width_plan.py that still runs blocks compact (COMPACT_CONFIGS), its 64-wide anchor nets and
# its classification net.  The anchor nets on the last block are 3x3 and 5x5 ones: the 96 x 144 frame of the re-shape leaves
# a 6 x 9 map there, which vgg_heads' 7x7 net does not fit.
FILTERS = WP.COMPACT_CONFIGS["backbone_64_128_192_320"]["filters"]
HEADS = [(3, 64, 3), (3, 64, 4), (5, 64, 4), (5, 64, 4)]
CLS = WP.COMPACT_CONFIGS["backbone_64_128_192_320"]["cls"]
FRAME = (128, 176)


def _model(F, seed=11):
    cfg = dict(F.duplo_cfg)
    model = F.create_model(cfg, WP.layers_of(FILTERS), WP.heads_of(HEADS), WP.cls_of(*CLS))
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=seed)
    return model, w, g


def _objective(F, model, w, g, H, W):
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=1)
    return F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))


def _step(F, model, f, w, seed):
    """One training step with device-drawn keep vectors at `seed`: (loss, gradient)."""
    import torch
    model["native"].seed = seed
    loss, grad = f(w)
    torch.cuda.synchronize()
    return loss, grad.cpu().numpy().copy()


def _compact_blocks(F, model):
    """Blocks the last training pass ran compact: the keep vectors it drew (debug buffer kind 4, as test_gpu_dropcompact
    reads them) through the shape rules of net.cpp plan_compact (width_plan.compact_plan)."""
    out = []
    for b, l in enumerate(model["layers"]):
        if l["dropout"] <= 0:
            continue
        p = C.c_void_p(); n = C.c_longlong()
        F._lib.call("frcnn_model_debug_buffer", model["native"].h, 4, b, C.byref(p), C.byref(n))
        keep = F.DeviceTensor(p.value, (l["filters"],), np.float32).numpy()
        assert set(np.unique(keep)) <= {0.0, 1.0}
        if WP.compact_plan(FILTERS, b, int(keep.sum())) == "compact":
            out.append(b)
    return out


def test_reshape_with_another_job_count_after_compact_passes(F):
    """Model A runs two training steps at 128 x 176 with compact blocks, then -- option split_bf16 off, so that no launch takes
    the split form and the table of split-operand pack jobs is empty -- one step at 96 x 144: the re-shape re-allocates the
    ring of per-step tables, whose events must start afresh.  Model B, made after the option change with the same weights,
    runs that third step only.  Loss and gradient are bit-equal.  Both final steps run in deterministic mode: the default
    mode's sums meet in fp32 atomics, whose order varies from run to run."""
    H, W = FRAME
    model_a, w_a, g_a = _model(F)
    f_a = _objective(F, model_a, w_a, g_a, H, W)
    opt = C.c_int()
    F._lib.call("frcnn_get_option", b"split_bf16", C.byref(opt))
    assert opt.value == 1
    try:
        for seed in (77, 78):
            _step(F, model_a, f_a, w_a, seed)
            assert _compact_blocks(F, model_a), "no block ran compact"
        F._lib.call("frcnn_set_option", b"split_bf16", 0)
        F._lib.call("frcnn_set_option", b"deterministic", 1)
        loss_a, grad_a = _step(F, model_a, _objective(F, model_a, w_a, g_a, 96, 144), w_a, 79)
        model_b, w_b, g_b = _model(F)
        assert np.array_equal(w_a.cpu().numpy(), w_b.cpu().numpy())
        loss_b, grad_b = _step(F, model_b, _objective(F, model_b, w_b, g_b, 96, 144), w_b, 79)
    finally:
        F._lib.call("frcnn_set_option", b"split_bf16", 1)
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    assert np.isfinite(loss_a) and np.abs(grad_a).max() > 0
    assert loss_a == loss_b, (loss_a, loss_b)
    assert np.array_equal(grad_a, grad_b), "%d gradient elements differ" % int((grad_a != grad_b).sum())


def _model_bytes_lower_bound(model, H, W):
    """Device memory one model certainly holds after a training step at H x W: every backbone convolution's output and that
    output's gradient (padding 1: the block's input size) and a packed copy of every weight tensor (param table kinds 0 and
    3: convolution and Linear weights)."""
    n = 0
    h, w = H, W
    for l in model["layers"]:
        n += l["conv_steps"] * 2 * l["filters"] * h * w * 4
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    n += sum(int(cnt) * 4 for off, cnt, kind, aux in model["native"].param_table if kind == 0)
    return n


def test_create_use_destroy_repeated(F):
    """Eight models in a row: created, one training step and one evaluate-mode forward, destroyed; every other one with the
    update stream armed (its passes record the events of frcnn_pnet_wait_block_done).  The device's free memory after the
    second and after the eighth differs by less than one model's buffers: nothing a model owns outlives it."""
    import torch
    H, W = FRAME
    free = {}
    bound = None
    for k in range(1, 9):
        model, w, g = _model(F)
        nat = model["native"]
        if k % 2 == 0:
            us = C.c_void_p()
            F._lib.call("frcnn_model_update_stream", nat.h, C.byref(us))
            assert us.value
        f = _objective(F, model, w, g, H, W)
        loss, grad = _step(F, model, f, w, 40 + k)
        assert np.isfinite(loss) and np.abs(grad).max() > 0
        model["pnet"].evaluate()
        outs = model["pnet"].forward(F.synthetic_image(H, W, k))
        torch.cuda.synchronize()
        assert all(np.isfinite(o.numpy()).all() for o in outs)
        bound = bound or _model_bytes_lower_bound(model, H, W)
        del outs, f, grad
        nat.__del__()   # frcnn_model_destroy, now
        assert nat.h is None
        del model, nat, w, g
        gc.collect()
        torch.cuda.synchronize()
        free[k] = torch.cuda.mem_get_info()[0]
    print("free memory after model 2: %d, after model 8: %d, bound %d" % (free[2], free[8], bound))
    assert abs(free[2] - free[8]) < bound, (free, bound)


def test_waits_for_events_never_recorded(F):
    """Before any backward pass frcnn_pnet_wait_heads_done and frcnn_pnet_wait_block_gradients are state errors;
    frcnn_cnet_backward_join and frcnn_pnet_anchor_loss_wait on a fresh model have nothing to wait for and succeed."""
    import torch
    model, w, g = _model(F)
    h = model["native"].h
    lib = F._lib.load()
    s = F.stream_ptr()
    with pytest.raises(F.FrcnnError, match="pnet_wait_heads_done: call frcnn_pnet_backward first"):
        F._lib.call("frcnn_pnet_wait_heads_done", h, s)
    with pytest.raises(F.FrcnnError, match="pnet_wait_block_gradients: call frcnn_pnet_backward first"):
        F._lib.call("frcnn_pnet_wait_block_gradients", h, 1, s)
    assert lib.frcnn_cnet_backward_join(h, s) == 0        # FRCNN_OK
    assert lib.frcnn_pnet_anchor_loss_wait(h, s) == 0
    torch.cuda.synchronize()
