"""Shared by tests/test_upscale.py (CPU) and tests/test_upscale_gpu.py: the small eval-mode generator of the exactness tests and
the fp64 oracle forward over its state dict.  Not a test module."""
import functools

import torch

from oracle import model as om

CH = 16


@functools.lru_cache(maxsize=None)
def generator_state(n_rcb: int, upscale: int):
    """A 16-channel generator with every eval-mode term alive: random running statistics, BatchNorm and conv biases; conv3 scaled
    by 0.02 with bias + 0.5 so that the output stays inside the clamp (fp32 tensors; callers must not modify them)."""
    torch.manual_seed(1000 * n_rcb + upscale)
    sd = om.init_generator_state(ch=CH, n_rcb=n_rcb, upscale=upscale)
    g = torch.Generator().manual_seed(7 * n_rcb + upscale)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    sd["conv3.weight"] = sd["conv3.weight"] * 0.02
    sd["conv3.bias"] = sd["conv3.bias"] + 0.5
    return sd


def oracle_forward(n_rcb: int, upscale: int):
    """x fp64 [B,3,h,w] -> the oracle's eval-mode forward in fp64."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in generator_state(n_rcb, upscale).items()}
    return lambda x: om.generator_forward(sd, x, training=False)


def lr_image(h: int, w: int, seed: int = 3):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def clamped_share(sr) -> float:
    """Share of the outputs that sit on the clamp's bounds."""
    return float(((sr <= 0) | (sr >= 1)).double().mean())
