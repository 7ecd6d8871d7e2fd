"""Shared by tests/test_grad_clip.py (CPU) and tests/test_grad_clip_gpu.py: the fp64 restatement of global gradient-norm clipping
and the non-finite guard of the flat Adam (csrc/optim.hip: sst_grad_sumsq / sst_adam_flat_clip).  Not a test module.

    norm = sqrt(sum of g^2 over the PARAMETER elements of the flat buffer)       (pad words excluded: ema_refs.slot_mask)
    coef = min(1, max_norm / (norm + 1e-6)), 1 when max_norm == 0               (torch.nn.utils.clip_grad_norm_)
    skip = guard on and the sum is not finite
    one Adam step (torch.optim.Adam, non-amsgrad) on g * coef."""
import math

import torch

from ema_refs import slot_mask


def norm_ref(g, offs, numels):
    """fp64 L2 norm of the parameter elements of the flat buffer g, summed sequentially (torch.sum of a double tensor is a
    tree; both are within (n - 1) * 2^-53 relative of the exact sum of the exact squares)."""
    mask = slot_mask(offs, numels, g.numel(), g.device)
    return math.sqrt(float(g[mask].double().square().sum()))


def coef_ref(norm, max_norm):
    if max_norm == 0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0          # NaN goes through, like torch.clamp


def clipped_adam_step_ref(p, g, m, v, t, lr, b1, b2, eps, wd, max_norm, skip_nonfinite=False):
    """One step on lists of fp64 tensors (p, g, m, v per parameter), t the step count BEFORE it.  Returns
    (p, m, v, t, norm, coef, skipped); the inputs are not modified."""
    total = sum(float(x.double().square().sum()) for x in g)
    norm = math.sqrt(total) if total == total and total >= 0 else float("nan")
    if skip_nonfinite and not math.isfinite(total):
        return [x.clone() for x in p], [x.clone() for x in m], [x.clone() for x in v], t, norm, 1.0, True
    coef = coef_ref(norm, max_norm)
    t = t + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    P, M, V = [], [], []
    for pi, gi, mi, vi in zip(p, g, m, v):
        gg = gi.double() * coef + wd * pi.double()
        mn = b1 * mi.double() + (1.0 - b1) * gg
        vn = b2 * vi.double() + (1.0 - b2) * gg * gg
        P.append(pi.double() - (lr / bc1) * mn / (vn.sqrt() / math.sqrt(bc2) + eps))
        M.append(mn)
        V.append(vn)
    return P, M, V, t, norm, coef, False
