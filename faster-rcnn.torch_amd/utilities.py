"""combine_and_flatten_parameters (utilities.lua:136-147) and the optimiser steps of
main.lua:122-124,133-135 (optim.rmsprop, optim.sgd, optim.nag).  The flat weight / gradient vectors are torch CUDA tensors so that
`torch.distributed` (RCCL) can all-reduce the gradient in place."""
import numpy as np

from . import _lib
from .tensor import ptr, stream_ptr


def combine_and_flatten_parameters(pnet, cnet, seed=42, weights_host=None):
    """-> weights, gradient: ONE contiguous device vector each (pnet parameters first, then cnet).
    Both nets are re-pointed at the flat storage (nn.Module.flatten semantics)."""
    import torch
    native = pnet.native
    assert cnet.native is native
    if not torch.cuda.is_available():
        raise _lib.FrcnnError("no HIP device: the product path has no CPU fallback")
    w0 = native.init_parameters(seed) if weights_host is None else np.asarray(weights_host, dtype=np.float32)
    assert w0.size == native.total_params
    weights = torch.from_numpy(w0).cuda()
    gradient = torch.zeros_like(weights)
    native.weights, native.gradient = weights, gradient
    nbn = native.bn_running_size()
    if nbn:
        bn = np.zeros(nbn, dtype=np.float32)
        o = 0
        for i in range(native.desc.ncls):
            if native.desc.cls_bn[i]:
                n = native.desc.cls_n[i]
                bn[o + n:o + 2 * n] = 1.0  # running_mean 0, running_var 1
                o += 2 * n
        native.bn_running = torch.from_numpy(bn).cuda()
    return weights, gradient


import os
EAGER_DEFAULT = os.environ.get("FRCNN_EAGER_UPDATE", "0") == "1"


def staged_ranges(opfunc):
    """The trainable slices the next pass of opfunc would train (create_objective's cfg["train"], validated now), or None:
    the whole vector (no staged training, or an opfunc that does not publish ranges)."""
    f = getattr(opfunc, "trainable_ranges", None)
    return f() if f is not None else None


def _state_vector(x, opfunc):
    """A fresh optimiser state vector whose first update writes every element it covers: zeros when the coming pass is
    staged, so that a frozen slice starts from 0 whenever it is trained later (it was never handed to the optimiser)."""
    import torch
    return torch.zeros_like(x) if staged_ranges(opfunc) is not None else torch.empty_like(x)


def _guard_config(config, state, name):
    """The gradient guard of a step (include/frcnn_hip.h "gradient-norm clipping"): config["clipNorm"] (a positive float: the L2
    norm the gradient handed to the optimiser may have at most; None or 0: no clipping) and config["skipNonFinite"] (bool; implied
    by a clipNorm: a step whose gradient holds an inf or a NaN treats it as zero).  Either one turns the guard on.
    -> None (off: the step queues what it always did) or the clip norm as a float (0.0: record the norm, clip nothing).
    Bad values raise ValueError, the guard together with state["eager"] FrcnnError, before any device call."""
    clip = config.get("clipNorm")
    skip = config.get("skipNonFinite")
    if clip is not None:
        if isinstance(clip, bool) or not isinstance(clip, (int, float, np.integer, np.floating)):
            raise ValueError("optim.%s: clipNorm must be a number, not %r" % (name, clip))
        clip = float(clip)
        if clip != clip or clip < 0 or clip == float("inf"):
            raise ValueError("optim.%s: clipNorm must be a finite number >= 0 (0: no clipping), not %r" % (name, clip))
    if skip is not None and not isinstance(skip, (bool, np.bool_)):
        raise ValueError("optim.%s: skipNonFinite must be a boolean, not %r" % (name, skip))
    if not clip and not skip:
        return None
    if state.get("eager", EAGER_DEFAULT):
        raise _lib.FrcnnError("optim.%s: clipNorm / skipNonFinite cannot be combined with the eager update: its slice-by-slice "
                              "update starts before the gradient's norm exists" % name)
    return clip or 0.0


def _guard_queue(state, x, dfdx, ranges, divisor, clip, record_ptr):
    """frcnn_grad_clip over `ranges` of dfdx (None: the whole vector) on the current stream; divisor None, a host count or a
    DeviceDivisor.  The workspace (and, without an objective that owns one, the record) lives in state["_guard"]."""
    import ctypes as C
    import torch
    n = x.numel()
    own = state.get("_guard")
    if own is None or own["n"] != n or own["ws"].device != x.device:
        nbytes = _lib.load().frcnn_grad_clip_workspace_bytes(n)
        own = state["_guard"] = dict(n=n, ws=torch.empty(nbytes // 8, dtype=torch.float64, device=x.device),
                                     record=torch.zeros(4, dtype=torch.float64, device=x.device))
    if record_ptr is None:
        record_ptr = own["record"].data_ptr()
    flat = None
    if ranges is not None:
        flat = (C.c_longlong * (2 * len(ranges)))(*[int(b) for r in ranges for b in r])
    ddev = ptr(divisor.ptr) if hasattr(divisor, "ptr") else None
    dhost = 1.0 if divisor is None or ddev is not None else float(divisor)
    _lib.call("frcnn_grad_clip", ptr(dfdx), n, flat, 0 if ranges is None else len(ranges), dhost, ddev, clip,
              C.c_void_p(record_ptr), ptr(own["ws"]), own["ws"].numel() * 8, stream_ptr())
    return record_ptr


def _step(opfunc, x, state, whole, update, guard=None):
    """One optimiser step around opfunc (main.lua:133-135), the update queued by the optimiser:
    whole(dfdx, gscale) updates the whole vector, gscale None (nothing to scale), a float (gradient:div(n), objective.lua:200,
    folded into the update's pass) or a DeviceDivisor (data parallel: the all-reduced count, still on the device);
    update(w, g, lo, hi, gscale, stream) is the same update on elements [lo, hi) (gscale 1: unscaled).
    Staged training (create_objective's cfg["train"]): only the slices the pass published (pass_ranges) are updated; a frozen
    slice keeps its weights and its optimiser state bit for bit, as if it had never been handed to the optimiser.
    guard (from _guard_config; None: off): frcnn_grad_clip is queued between the pass and the update, and the update runs with the
    device divisor D' of the guard's record (update() then receives a DeviceDivisor).  With create_objective's closure the record
    lives beside its accumulators and finish() reports stats["gnorm"] / stats["skipped"]; with a plain opfunc D = 1 and the
    record stays on the device in state["_guard"]["record"].
    Returns x, [f(x)] like the Lua functions."""
    begin = getattr(opfunc, "begin_fold", None)
    armed = None
    if guard is not None and begin is not None:
        arm = getattr(opfunc, "guard_arm", None)
        if arm is None:
            raise _lib.FrcnnError("clipNorm / skipNonFinite: this objective keeps no record for the gradient guard (no guard_arm)")
        armed = arm()
    timing = state.get("_timing")     # bench.py: seconds the host spends queueing a step / waiting for its statistics
    if timing is not None:
        import time
        t_in = time.perf_counter()
    if begin is not None:   # create_objective's closure: the loss is read back AFTER the update has been queued,
        # and gradient:div(n) rides on the update's own pass over the vectors.  state["eager"] (default off: measured neutral on
        # one GPU, EXPERIMENTS.md round 6 -- the backward pass has no idle registers for the update to run in): the pass may
        # apply this very step slice by slice, beside its own backward half, as slices of the gradient become final
        eager = dict(update=update) if state.get("eager", EAGER_DEFAULT) else None   # (never with the guard: _guard_config)
        finish, dfdx, gscale = begin(x, eager) if eager is not None else begin(x)
        pass_ranges = getattr(opfunc, "pass_ranges", None)
        ranges = pass_ranges() if pass_ranges is not None else None
        if armed is not None:
            _guard_queue(state, x, dfdx, ranges, armed.divisor(), guard, armed.ptr)
            armed.queued()
            gscale = armed.record
        if eager is not None and "done" in eager:
            # what the pass has not updated (the shallowest block: its gradients end the pass; everything, for an image without
            # examples) -- of the trainable slices -- on the caller's stream, followed by the packs made from it
            from .objective import uncovered
            for lo, hi in uncovered(eager["done"], eager.get("ranges") or [(0, x.numel())]):
                eager["slice"](lo, hi, stream_ptr())
            eager["complete"]()
        elif ranges is not None:
            for lo, hi in ranges:   # (gscale: a host factor, or a DeviceDivisor -> the _slice_dev forms)
                update(x, dfdx, lo, hi, 1.0 if gscale is None else gscale, stream_ptr())
        else:
            whole(dfdx, gscale)
        if timing is not None:
            t_q = time.perf_counter()
        fx, _ = finish()
        if timing is not None:
            timing["enqueue"] += t_q - t_in; timing["wait"] += time.perf_counter() - t_q; timing["steps"] += 1
        return x, [fx]
    fx, dfdx = opfunc(x)
    if guard is not None:
        from .objective import DeviceDivisor
        rec = _guard_queue(state, x, dfdx, None, None, guard, None)
        whole(dfdx, DeviceDivisor(rec + 2 * 8, state["_guard"]["record"]))
        return x, [fx]
    whole(dfdx, None)
    return x, [fx]


def _fold_args(gscale):
    """(gscale, gcount_dev) of frcnn_sgd / frcnn_nag for what begin_fold returned as the divisor"""
    if hasattr(gscale, "ptr"):
        return 1.0, ptr(gscale.ptr)
    return (1.0 if gscale is None else gscale), None


def rmsprop(opfunc, x, state):
    """optim.rmsprop(opfunc, x, state) [ext]: state.learningRate (1e-2), state.alpha (0.99),
    state.epsilon (1e-8); m = alpha*m + (1-alpha)*g^2 ; x -= lr * g / (sqrt(m) + eps).
    Returns x, [f(x)] like the Lua function (main.lua:133)."""
    import torch
    lr = state.get("learningRate", 1e-2); alpha = state.get("alpha", 0.99); eps = state.get("epsilon", 1e-8)
    guard = _guard_config(state, state, "rmsprop")
    if "m" not in state:
        state["m"] = torch.zeros_like(x)
    m = state["m"]

    def whole(dfdx, gscale):
        if hasattr(gscale, "ptr"):
            _lib.call("frcnn_scale_rmsprop_dev", ptr(x), ptr(dfdx), ptr(gscale.ptr), ptr(m), x.numel(), lr, alpha, eps, stream_ptr())
        elif gscale is None:
            _lib.call("frcnn_rmsprop", ptr(x), ptr(dfdx), ptr(m), x.numel(), lr, alpha, eps, stream_ptr())
        else:
            _lib.call("frcnn_scale_rmsprop", ptr(x), ptr(dfdx), gscale, ptr(m), x.numel(), lr, alpha, eps, stream_ptr())

    def update(w, g, lo, hi, gscale, on):
        if hasattr(gscale, "ptr"):
            _lib.call("frcnn_scale_rmsprop_slice_dev", ptr(w), ptr(g), ptr(gscale.ptr), ptr(m), lo, hi, lr, alpha, eps, on)
        else:
            _lib.call("frcnn_scale_rmsprop_slice", ptr(w), ptr(g), gscale, ptr(m), lo, hi, lr, alpha, eps, on)
    return _step(opfunc, x, state, whole, update, guard)


def _get(config, key, default):
    v = config.get(key)      # (Lua: `config.key or default`)
    return default if v is None else v


def _no_per_parameter(config, name):
    if config.get("learningRates") is not None or config.get("weightDecays") is not None:
        raise ValueError("optim.%s: per-parameter learningRates / weightDecays are not supported by the device optimiser "
                         "(give the scalar learningRate / weightDecay)" % name)


def sgd(opfunc, x, config, state=None):
    """optim.sgd(opfunc, x, config[, state]) [ext] (main.lua:122-124 sgd_state, :135): config.learningRate (1e-3),
    learningRateDecay (0), weightDecay (0), momentum (0), dampening (= momentum), nesterov (false).  g += wd*x;
    v = g on the first step, else v = v*mom + (1-damp)*g (state["dfdx"]); g += mom*v (nesterov) and x -= clr*g, else x -= clr*v;
    clr = lr / (1 + evalCounter*lrd).  One pass of frcnn_sgd.  Returns x, [f(x)] like the Lua function."""
    import torch
    state = config if state is None else state
    lr = _get(config, "learningRate", 1e-3); lrd = _get(config, "learningRateDecay", 0)
    wd = _get(config, "weightDecay", 0); mom = _get(config, "momentum", 0)
    damp = _get(config, "dampening", mom); nesterov = bool(_get(config, "nesterov", False))
    _no_per_parameter(config, "sgd")
    guard = _guard_config(config, state, "sgd")
    if nesterov and not (mom > 0 and damp == 0):
        raise ValueError("optim.sgd: Nesterov momentum requires a momentum and zero dampening")
    nevals = state.get("evalCounter") or 0
    clr = lr / (1 + nevals * lrd)           # host scalars in double, as Lua computes them
    first = mom != 0 and "dfdx" not in state
    if first:
        state["dfdx"] = _state_vector(x, opfunc)   # (its contents are the kernel's: v = copy(g))
    v = state["dfdx"] if mom != 0 else None
    args = (wd, mom, 1 - damp, int(nesterov), int(first))

    def whole(dfdx, gscale):
        gs, gcount = _fold_args(gscale)
        _lib.call("frcnn_sgd", ptr(x), ptr(dfdx), ptr(v), x.numel(), gs, gcount, clr, *args, stream_ptr())

    def update(w, g, lo, hi, gscale, on):
        if hasattr(gscale, "ptr"):
            _lib.call("frcnn_sgd_slice_dev", ptr(w), ptr(g), ptr(v), lo, hi, ptr(gscale.ptr), clr, *args, on)
        else:
            _lib.call("frcnn_sgd_slice", ptr(w), ptr(g), ptr(v), lo, hi, gscale, clr, *args, on)
    try:
        r = _step(opfunc, x, state, whole, update, guard)
    except BaseException:
        if first:
            del state["dfdx"]
        raise
    state["evalCounter"] = nevals + 1
    return r


def nag(opfunc, x, config, state=None):
    """optim.nag(opfunc, x, config[, state]) [ext] (main.lua:124 nag_state, :134): config.learningRate (1e-3),
    learningRateDecay (0), weightDecay (0), momentum (0.9, must be > 0).  The look-ahead x += mom*v (when state["dfdx"]
    exists) before opfunc, then g += wd*x; v = 0 on the first step, else v = v*mom; v -= clr*g; x += v.
    clr = lr / (1 + evalCounter*lrd).  Returns x, [f(x)] like the Lua function."""
    import torch
    from torch.autograd.graph import increment_version
    state = config if state is None else state
    lr = _get(config, "learningRate", 1e-3); lrd = _get(config, "learningRateDecay", 0)
    wd = _get(config, "weightDecay", 0); mom = _get(config, "momentum", 0.9)
    if mom <= 0:
        raise ValueError("optim.nag: momentum must be positive for Nesterov Accelerated Gradient")
    _no_per_parameter(config, "nag")
    guard = _guard_config(config, state, "nag")
    nevals = state.get("evalCounter") or 0
    clr = lr / (1 + nevals * lrd)
    first = "dfdx" not in state
    if first:
        state["dfdx"] = _state_vector(x, opfunc)   # (fill(0) is folded into the first update)
    else:
        ranges = staged_ranges(opfunc)
        if ranges is None:
            _lib.call("frcnn_nag_lookahead", ptr(x), ptr(state["dfdx"]), x.numel(), mom, stream_ptr())
        else:   # staged training: a frozen slice keeps its weights
            for lo, hi in ranges:
                _lib.call("frcnn_nag_lookahead_slice", ptr(x), ptr(state["dfdx"]), lo, hi, mom, stream_ptr())
        # torch does not see the library's write: counting it as torch's own makes create_objective withdraw a pack promise
        # made for the weights before the look-ahead (frcnn_pnet_invalidate_packs) instead of forwarding with stale packs
        increment_version(x)
    v = state["dfdx"]
    args = (wd, mom, int(first))

    def whole(dfdx, gscale):
        gs, gcount = _fold_args(gscale)
        _lib.call("frcnn_nag", ptr(x), ptr(dfdx), ptr(v), x.numel(), gs, gcount, clr, *args, stream_ptr())

    def update(w, g, lo, hi, gscale, on):
        if hasattr(gscale, "ptr"):
            _lib.call("frcnn_nag_slice_dev", ptr(w), ptr(g), ptr(v), lo, hi, ptr(gscale.ptr), clr, *args, on)
        else:
            _lib.call("frcnn_nag_slice", ptr(w), ptr(g), ptr(v), lo, hi, gscale, clr, *args, on)
    try:
        r = _step(opfunc, x, state, whole, update, guard)
    except BaseException:
        if first:
            del state["dfdx"]
        raise
    state["evalCounter"] = nevals + 1
    return r


def adam(opfunc, x, config, state=None):
    """optim.adam(opfunc, x, config[, state]) [ext] (Torch's optim/adam.lua): config.learningRate (1e-3), learningRateDecay (0),
    beta1 (0.9), beta2 (0.999), epsilon (1e-8), weightDecay (0), and decoupled (False; not in Torch: weightDecay becomes
    AdamW's decay x -= clr*weightDecay*x, which the gradient and the moments never see, instead of Torch's g += wd*x).
    m = m*beta1 + (1-beta1)*g ; v = v*beta2 + (1-beta2)*g*g ; x -= stepSize * m / (sqrt(v) + eps) with
    clr = lr / (1 + t*lrd), t += 1, stepSize = clr * sqrt(1 - beta2^t) / (1 - beta1^t); state["t"], state["m"], state["v"]
    (zeros before the first step).  One pass of frcnn_adam.  Bad values raise ValueError before x or opfunc is touched; a
    step that raises leaves the state as it was.  Returns x, [f(x)] like the Lua function."""
    import math
    import torch
    state = config if state is None else state
    lr = _get(config, "learningRate", 1e-3); lrd = _get(config, "learningRateDecay", 0)
    beta1 = _get(config, "beta1", 0.9); beta2 = _get(config, "beta2", 0.999)
    eps = _get(config, "epsilon", 1e-8); wd = _get(config, "weightDecay", 0)
    decoupled = _get(config, "decoupled", False)
    for key, beta in (("beta1", beta1), ("beta2", beta2)):
        if not 0 <= beta < 1:
            raise ValueError("optim.adam: %s must lie in [0, 1), not %r" % (key, beta))
    if not eps > 0:
        raise ValueError("optim.adam: epsilon must be positive, not %r" % (eps,))
    if not lr >= 0:
        raise ValueError("optim.adam: learningRate must not be negative, not %r" % (lr,))
    if not wd >= 0:
        raise ValueError("optim.adam: weightDecay must not be negative, not %r" % (wd,))
    if not isinstance(decoupled, (bool, np.bool_)):
        raise ValueError("optim.adam: decoupled must be a boolean, not %r" % (decoupled,))
    _no_per_parameter(config, "adam")
    guard = _guard_config(config, state, "adam")
    t = state.get("t") or 0
    clr = lr / (1 + t * lrd)                # host scalars in double, as Lua computes them (the t from before the increment)
    t += 1
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    step = clr * math.sqrt(bc2) / bc1
    coupled, decay = (0.0, clr * wd) if decoupled else (wd, 0.0)
    created = [key for key in ("m", "v") if key not in state]
    for key in created:
        state[key] = torch.zeros_like(x)    # (zeros always: every step reads both, and a frozen slice keeps them)
    m, v = state["m"], state["v"]
    args = (step, beta1, 1 - beta1, beta2, 1 - beta2, eps, coupled, decay)

    def whole(dfdx, gscale):
        gs, gcount = _fold_args(gscale)
        _lib.call("frcnn_adam", ptr(x), ptr(dfdx), ptr(m), ptr(v), x.numel(), gs, gcount, *args, stream_ptr())

    def update(w, g, lo, hi, gscale, on):
        if hasattr(gscale, "ptr"):
            _lib.call("frcnn_adam_slice_dev", ptr(w), ptr(g), ptr(m), ptr(v), lo, hi, ptr(gscale.ptr), *args, on)
        else:
            _lib.call("frcnn_adam_slice", ptr(w), ptr(g), ptr(m), ptr(v), lo, hi, gscale, *args, on)
    try:
        r = _step(opfunc, x, state, whole, update, guard)
    except BaseException:
        for key in created:
            del state[key]
        raise
    state["t"] = t
    return r


_OPTIMIZERS = dict(rmsprop=rmsprop, sgd=sgd, nag=nag)


def optimizer(name):
    """The optimiser function for a value of main.lua's -opti (main.lua:35): 'rmsprop' (its default), 'sgd' or 'nag'.
    This stays the table of main.lua's values: optim.adam is not one of them, so optimizer("adam") raises ValueError --
    call F.adam directly."""
    try:
        return _OPTIMIZERS[name]
    except KeyError:
        raise ValueError("unknown optimiser %r (main.lua -opti: %s)" % (name, ", ".join(sorted(_OPTIMIZERS))))


def reverse(array):  # utilities.lua:79-87
    array.reverse()
    return array
