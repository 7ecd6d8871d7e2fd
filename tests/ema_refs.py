"""Shared by tests/test_checkpoint.py (CPU), tests/test_ema_gpu.py and tests/test_resume_gpu.py: the fp64 restatement of the
parameter average the flat Adam kernel keeps (csrc/optim.hip), and the helpers that compare against it.  Not a test module.

The rule, with t the Adam step count of the update (1 at the first step):
    d   = min(decay, (1 + t) / (10 + t)) with warm-up, else decay
    ema = fp32(d * ema + (1 - d) * p_new), evaluated in fp64 and rounded once."""
import torch


def decay_at(t, decay, warmup):
    t = float(t)
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def ema_ref(ema, p_new, t, decay, warmup):
    d = decay_at(t, decay, warmup)
    return (d * ema.double() + (1.0 - d) * p_new.double()).float()


def _ordered(x):
    """fp32 bit patterns through the int32 view as integers that order like the floats (-0 and +0 coincide)."""
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    """Largest distance between two fp32 tensors in units in the last place."""
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    return int((_ordered(a) - _ordered(b)).abs().max())


def slot_mask(offs, numels, total, device):
    """True on the words of a flat buffer (ops.flat_layout) that belong to a parameter, False on the pad words."""
    mask = torch.zeros(total, dtype=torch.bool, device=device)
    for o, n in zip(offs, numels):
        mask[o:o + n] = True
    return mask


def equal_tree(a, b):
    """Recursive equality of checkpoint contents: tensors with torch.equal (same dtype), containers element-wise, scalars ==."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a.cpu(), b.cpu()))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(equal_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(equal_tree(x, y) for x, y in zip(a, b))
    return a == b
