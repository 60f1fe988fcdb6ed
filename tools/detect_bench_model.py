"""The model tools/bench_detect_batch.py and tools/bench_detect_mixed.py time: vgg_small under the duplo settings with weights
amplified as bench.py's inference leg -- the head convolutions' class logits x `gain`, so that anchors pass p > 0.95, and the
class head x200, so that candidates pass p > 0.2."""
import torch


def amplified_vgg_small(F, gain):
    """-> (cfg, model, weights, gradient); `weights` (kept alive by the caller) holds the amplified values"""
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    for off, cnt, kind, aux in model["native"].param_table:
        if kind == 0 and aux == 18:
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= gain
        if kind == 3 and cnt == 512 * (cfg["class_count"] + 1):
            w[off:off + cnt] *= 200.0
    weights.copy_(torch.from_numpy(w))
    return cfg, model, weights, gradient
