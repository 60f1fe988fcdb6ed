"""Data-parallel optim.adam step on real kernels: two gloo ranks share the one GPU, rank r takes image r, and the fused update
reads the all-reduced example count on the device (frcnn_adam's gcount_dev, the divisor of objective.lua:200).  The result must
equal the single-process step on the two-image batch, to the tolerances test_gpu_optim_dp.py uses for optim.sgd.  (The helpers
follow that file, copied so that the two stand alone.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 176
ADAM_STATE = dict(learningRate=1e-3, weightDecay=0.0005)


def _setup():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frcnn_amd as F
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    anchors = F.Anchors(model["pnet"], cfg["scales"])
    sizes = F.output_map_sizes(model, H, W)
    images = []
    mt = F.MT19937(7)
    for k in range(2):
        rois = F.synthetic_rois(cfg, W, H, 3, 7, k)
        pos, neg = F.assemble_examples(anchors, cfg, rois, W, H, mt, negatives=8)
        pos, neg = F.clean_examples(pos, sizes), F.clean_examples(neg, sizes)
        images.append(dict(img=F.synthetic_image(H, W, k), positive=pos, negative=neg))
    rng = np.random.RandomState(3)
    pm = [None if l["dropout"] <= 0 else (rng.rand(l["filters"]) > l["dropout"]).astype(np.float32) for l in model["layers"]]
    cms = []
    for x in images:
        R = len(x["positive"]) + len(x["negative"])
        cms.append([(rng.rand(R, 1024) > 0.5).astype(np.float32), (rng.rand(R, 512) > 0.5).astype(np.float32)])
    return F, model, weights, gradient, images, pm, cms


class _Batch(object):
    def __init__(self, batch):
        self.batch = batch

    def nextTraining(self, count=None):
        return self.batch


def _step(F, model, weights, gradient, batch, pm, cms):
    """one F.adam step with coupled weight decay and explicit dropout masks (one cnet mask set per image, in order)
    -> the statistics and the two moment vectors"""
    model["pnet"].drop_masks = pm
    cnet = model["cnet"]
    orig = cnet.forward
    it = iter(cms)

    def fwd(x):
        cnet.drop_masks = next(it)
        return orig(x)
    cnet.forward = fwd
    state = dict(ADAM_STATE)
    try:
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, weights, gradient, _Batch(batch), stats)
        F.adam(f, weights, state)
    finally:
        cnet.forward = orig
        cnet.drop_masks = None
        model["pnet"].drop_masks = None
    assert state["t"] == 1
    return [stats[k][-1] for k in ("pcls", "preg", "dcls", "dreg")], state["m"], state["v"]


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    F, model, weights, gradient, images, pm, cms = _setup()
    st, m, v = _step(F, model, weights, gradient, [images[rank]], pm, [cms[rank]])
    torch.cuda.synchronize()
    for name, a in (("g", gradient), ("w", weights), ("m", m), ("v", v)):
        np.save(os.path.join(out_dir, "%s%d.npy" % (name, rank)), a.cpu().numpy())
    np.save(os.path.join(out_dir, "s%d.npy" % rank), np.array(st))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_adam_step_equals_single_process(tmp_path):
    import torch.multiprocessing as mp
    port = 29800 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = dict((k, np.load(tmp_path / ("%s0.npy" % k))) for k in "gwmvs")
    r1 = dict((k, np.load(tmp_path / ("%s1.npy" % k))) for k in "gwmvs")
    for k in "gwmvs":
        assert np.array_equal(r0[k], r1[k]), "the replicas differ in %s" % k
    F, model, weights, gradient, images, pm, cms = _setup()
    w_init = weights.cpu().numpy().copy()
    st, m, v = _step(F, model, weights, gradient, images, pm, cms)
    g = gradient.cpu().numpy(); w = weights.cpu().numpy(); m = m.cpu().numpy(); v = v.cpu().numpy()
    err_g = np.linalg.norm(r0["g"] - g) / np.linalg.norm(g)
    err_m = np.linalg.norm(r0["m"] - m) / np.linalg.norm(m)
    err_v = np.linalg.norm(r0["v"] - v) / np.linalg.norm(v)
    err_w = np.linalg.norm(r0["w"] - w) / np.linalg.norm(w - w_init)
    print("adam dp: relative L2 error of g %.3g, m %.3g, v %.3g, of the weights' step %.3g" % (err_g, err_m, err_v, err_w))
    assert np.allclose(r0["s"], st, rtol=1e-6, atol=0)
    # the gradient holds the scaled gradient plus wd*x; the first step's moments are (1-beta1)*g and (1-beta2)*g*g of it
    assert err_g <= 1e-5 and err_m <= 1e-5 and err_v <= 1e-5
    f32 = np.float32
    assert np.array_equal(m, f32(1 - 0.9) * g) and np.array_equal(r0["m"], f32(1 - 0.9) * r0["g"])
    assert np.array_equal(v, (f32(1 - 0.999) * g) * g) and np.array_equal(r0["v"], (f32(1 - 0.999) * r0["g"]) * r0["g"])
    assert np.abs(w - w_init).max() > 0
    assert err_w <= 1e-3
