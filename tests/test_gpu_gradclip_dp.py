"""The gradient guard in the data-parallel optim.sgd step: two gloo ranks share the one GPU, rank r takes image r, the flat
gradient and the example count are all-reduced, and every rank then runs frcnn_grad_clip on its (identical) reduced gradient with
the all-reduced count as the device divisor D.  S is summed in a fixed order, so the ranks compute the same S, the same D' and
stay replicas bit for bit; the result must equal the single-process guarded step on the two-image batch.  clipNorm is half the
norm the single-process step records.  (The helpers follow test_gpu_optim_dp.py, copied so that the files stand alone.)"""
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


def _step(F, model, weights, gradient, batch, pm, cms, guard):
    """one F.sgd step with main.lua's sgd_state plus the guard's keys and explicit dropout masks (one cnet mask set per image,
    in order) -> the statistics (the four losses, then gnorm), the momentum vector, the number of skipped steps"""
    model["pnet"].drop_masks = pm
    cnet = model["cnet"]
    orig = cnet.forward
    it = iter(cms)

    def fwd(x):
        cnet.drop_masks = next(it)
        return orig(x)
    cnet.forward = fwd
    state = dict(SGD_STATE, **guard)
    try:
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, weights, gradient, _Batch(batch), stats)
        F.sgd(f, weights, state)
    finally:
        cnet.forward = orig
        cnet.drop_masks = None
        model["pnet"].drop_masks = None
    assert state["evalCounter"] == 1
    assert len(stats["gnorm"]) == 1
    return [stats[k][-1] for k in ("pcls", "preg", "dcls", "dreg", "gnorm")], state["dfdx"], stats["skipped"]


def _worker(rank, world, port, out_dir, clip):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    F, model, weights, gradient, images, pm, cms = _setup()
    st, v, skipped = _step(F, model, weights, gradient, [images[rank]], pm, [cms[rank]], dict(clipNorm=clip))
    assert skipped == 0
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, "g%d.npy" % rank), gradient.cpu().numpy())
    np.save(os.path.join(out_dir, "w%d.npy" % rank), weights.cpu().numpy())
    np.save(os.path.join(out_dir, "v%d.npy" % rank), v.cpu().numpy())
    np.save(os.path.join(out_dir, "s%d.npy" % rank), np.array(st))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_clipped_sgd_step_equals_single_process(tmp_path):
    import torch.multiprocessing as mp
    # the single-process norm of the two-image batch (a guard that records and clips nothing)
    F, model, weights, gradient, images, pm, cms = _setup()
    probe, _, skipped = _step(F, model, weights, gradient, images, pm, cms, dict(skipNonFinite=True))
    norm = probe[4]
    assert np.isfinite(norm) and norm > 0 and skipped == 0
    clip = 0.5 * norm
    port = 29900 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, str(tmp_path), clip), nprocs=2, join=True)
    g0, g1 = np.load(tmp_path / "g0.npy"), np.load(tmp_path / "g1.npy")
    w0, w1 = np.load(tmp_path / "w0.npy"), np.load(tmp_path / "w1.npy")
    v0, v1 = np.load(tmp_path / "v0.npy"), np.load(tmp_path / "v1.npy")
    s0, s1 = np.load(tmp_path / "s0.npy"), np.load(tmp_path / "s1.npy")
    assert np.array_equal(g0, g1) and np.array_equal(w0, w1) and np.array_equal(v0, v1) and np.array_equal(s0, s1)   # replicas
    F, model, weights, gradient, images, pm, cms = _setup()
    w_init = weights.cpu().numpy().copy()
    st, v, skipped = _step(F, model, weights, gradient, images, pm, cms, dict(clipNorm=clip))
    assert skipped == 0 and abs(st[4] - norm) <= 1e-5 * norm   # (the default mode's sums are not bit-reproducible run to run)
    g = gradient.cpu().numpy(); w = weights.cpu().numpy(); v = v.cpu().numpy()
    assert np.allclose(s0[:4], st[:4], rtol=1e-6, atol=0)
    print("gnorm: ranks %r, single process %r, relative difference %.3g" % (s0[4], st[4], abs(s0[4] - st[4]) / st[4]))
    assert abs(s0[4] - st[4]) <= 1e-5 * st[4]
    # the gradient holds the scaled gradient plus wd*x, and the first step's momentum vector is a copy of it
    assert np.linalg.norm(g0 - g) <= 1e-5 * np.linalg.norm(g)
    assert np.array_equal(v0, g0) and np.array_equal(v, g)
    assert np.abs(w - w_init).max() > 0
    assert np.linalg.norm(w0 - w) <= 1e-3 * np.linalg.norm(w - w_init)
