"""Data-parallel optim.sgd step (main.lua:122-123 sgd_state, :135) on real kernels: two gloo ranks share the one GPU, rank r
takes image r, and the fused update reads the all-reduced example count on the device (frcnn_sgd's gcount_dev, the divisor of
objective.lua:200).  The result must equal the single-process step on the two-image batch.  (The helpers follow
test_gpu_dp.py, copied so that the two files stand alone.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 176
SGD_STATE = dict(learningRate=1e-3, weightDecay=0.0005, momentum=0.9)   # main.lua:122-123


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
    """one F.sgd step with main.lua's sgd_state and explicit dropout masks (one cnet mask set per image, in order)
    -> the statistics and the momentum vector"""
    model["pnet"].drop_masks = pm
    cnet = model["cnet"]
    orig = cnet.forward
    it = iter(cms)

    def fwd(x):
        cnet.drop_masks = next(it)
        return orig(x)
    cnet.forward = fwd
    state = dict(SGD_STATE)
    try:
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, weights, gradient, _Batch(batch), stats)
        F.sgd(f, weights, state)
    finally:
        cnet.forward = orig
        cnet.drop_masks = None
        model["pnet"].drop_masks = None
    assert state["evalCounter"] == 1
    return [stats[k][-1] for k in ("pcls", "preg", "dcls", "dreg")], state["dfdx"]


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    F, model, weights, gradient, images, pm, cms = _setup()
    st, v = _step(F, model, weights, gradient, [images[rank]], pm, [cms[rank]])
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, "g%d.npy" % rank), gradient.cpu().numpy())
    np.save(os.path.join(out_dir, "w%d.npy" % rank), weights.cpu().numpy())
    np.save(os.path.join(out_dir, "v%d.npy" % rank), v.cpu().numpy())
    np.save(os.path.join(out_dir, "s%d.npy" % rank), np.array(st))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_sgd_step_equals_single_process(tmp_path):
    import torch.multiprocessing as mp
    port = 29800 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g0, g1 = np.load(tmp_path / "g0.npy"), np.load(tmp_path / "g1.npy")
    w0, w1 = np.load(tmp_path / "w0.npy"), np.load(tmp_path / "w1.npy")
    v0, v1 = np.load(tmp_path / "v0.npy"), np.load(tmp_path / "v1.npy")
    s0, s1 = np.load(tmp_path / "s0.npy"), np.load(tmp_path / "s1.npy")
    assert np.array_equal(g0, g1) and np.array_equal(w0, w1) and np.array_equal(v0, v1) and np.array_equal(s0, s1)   # replicas
    F, model, weights, gradient, images, pm, cms = _setup()
    w_init = weights.cpu().numpy().copy()
    st, v = _step(F, model, weights, gradient, images, pm, cms)
    g = gradient.cpu().numpy(); w = weights.cpu().numpy(); v = v.cpu().numpy()
    assert np.allclose(s0, st, rtol=1e-6, atol=0)
    # the gradient holds the scaled gradient plus wd*x, and the first step's momentum vector is a copy of it
    assert np.linalg.norm(g0 - g) <= 1e-5 * np.linalg.norm(g)
    assert np.array_equal(v0, g0) and np.array_equal(v, g)
    assert np.abs(w - w_init).max() > 0
    assert np.linalg.norm(w0 - w) <= 1e-3 * np.linalg.norm(w - w_init)
