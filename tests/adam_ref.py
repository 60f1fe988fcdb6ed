"""optim.adam (Torch's optim/adam.lua) and AdamW's decoupled decay restated in numpy fp32, for the Adam tests: one separately
rounded numpy operation per Lua statement (numpy never contracts to FMA; np.sqrt and / on float32 are correctly rounded, as
they are on the device), host scalars in double as Lua computes them, cast with np.float32 where the library takes a float."""
import math

import numpy as np

f32 = np.float32


def adam_scalars(cfg, t):
    """the scalars of the step that finds state.t == t (t = 0: the first step) -> what frcnn_adam is handed"""
    lr = cfg.get("learningRate", 1e-3); lrd = cfg.get("learningRateDecay", 0)
    beta1 = cfg.get("beta1", 0.9); beta2 = cfg.get("beta2", 0.999)
    wd = cfg.get("weightDecay", 0)
    clr = lr / (1 + t * lrd)                                 # the t from before the increment
    t = t + 1
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    decoupled = bool(cfg.get("decoupled", False))
    return dict(step=clr * math.sqrt(bc2) / bc1, beta1=beta1, omb1=1 - beta1, beta2=beta2, omb2=1 - beta2,
                eps=cfg.get("epsilon", 1e-8), wd=0.0 if decoupled else wd, decay=clr * wd if decoupled else 0.0)


def ref_adam(x, g, m, v, gscale, s):
    """optim.adam after opfunc (gscale None: the gradient arrives divided) -> x, g, m, v as Torch leaves them"""
    if gscale is not None:
        g = g * f32(gscale)                                  # gradient:div(n)
    if s["wd"] != 0:
        g = g + f32(s["wd"]) * x                             # dfdx:add(wd, x)
    m = m * f32(s["beta1"]) + f32(s["omb1"]) * g             # state.m:mul(beta1):add(1-beta1, dfdx)
    v = v * f32(s["beta2"]) + (f32(s["omb2"]) * g) * g       # state.v:mul(beta2):addcmul(1-beta2, dfdx, dfdx)
    d = np.sqrt(v) + f32(s["eps"])                           # state.denom:copy(state.v):sqrt():add(epsilon)
    if s["decay"] != 0:
        x = x + f32(-s["decay"]) * x                         # AdamW: x -= clr*weightDecay*x
    x = x + (f32(-s["step"]) * m) / d                        # x:addcdiv(-stepSize, state.m, state.denom)
    return x, g, m, v


def adam_args(s):
    """the tail of frcnn_adam / frcnn_adam_slice / frcnn_adam_slice_dev between the divisor and the stream"""
    return (s["step"], s["beta1"], s["omb1"], s["beta2"], s["omb2"], s["eps"], s["wd"], s["decay"])


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gradient(rng, n):
    g = (rng.randn(n) * 3.0).astype(np.float32)
    g[::7] = 0.0                                             # signed zeros: 0 * anything, 0 + -0
    g[3::11] = -0.0
    return g
