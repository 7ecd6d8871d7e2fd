"""What the GPU tests of the structure-tensor family (tests/test_st_loss_fp64_gpu.py, test_st_general_gpu.py, test_st_maps_gpu.py)
share: inputs, the HIP and oracle sides of the loss and of the maps, and the fp64-truth rule applied to them.  A plain helper module.

fp64-truth rule (conftest): loss / per-image distance  |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads / map planes         rel_err(hip, o64) <= max(1e-3, 3 rel_err(o32, o64))
where l32 / o32 come from the fp32 oracle (the reference's arithmetic) and l64 / o64 from the same oracle in fp64."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err, truth_bound

UP = 0.7                                              # non-unit upstream gradient throughout
BUILDS = {(2, 8): (0.5, 2.0), (4, 10): (1.0, 2.5)}   # the two instantiated <R1, R2> pairs -> a (sigma, rho) that selects each
ALL = ("Sx", "Sgt", "Fx", "Fgt", "d", "tile_sums", "distance")


def radius_of(s):
    """csrc/st_tile.h radius_of: the kernel sees sigma / rho as fp32."""
    return max(int(4.0 * float(np.float32(s)) + 0.5), 1)


def images(seed, B, H, W, noise=0.08, scale=1.0):
    """Smooth texture (bicubic-upsampled noise) for gt and gt + noise for sr, both in [0, 1] x scale."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(H // 6, 2), max(W // 6, 2), generator=gen)
    gt = F.interpolate(base, size=(H, W), mode="bicubic", align_corners=False)
    gt = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    x = (gt + noise * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    return x * scale, gt * scale


# ------------------------------------------------------------------------------------------------ the loss
def loss_hip(x, gt, sigma, rho, norm):
    from srganst.loss import StructureTensorLoss
    xg = x.cuda().requires_grad_(True)
    loss = StructureTensorLoss(sigma, rho, norm)(xg, gt.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def loss_oracle(x, gt, sigma, rho, norm):
    from oracle import st as ost
    l32, g32 = ost.st_loss_and_grad(x, gt, sigma, rho, norm)
    l64, g64 = ost.st_loss_and_grad(x.double(), gt.double(), sigma, rho, norm)
    return l32.double(), g32.double(), l64, g64


def check_loss(name, hip, ref, grad=True):
    """Applies the fp64-truth rule to (loss, grad) and prints the measured errors."""
    (lh, gh), (l32, g32, l64, g64) = hip, ref
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_g, b_g = rel_err(gh, g64), truth_bound(g32, g64)
    print(f"[{name}] loss {lh.item():.6e} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err {e_g:.3e} <= {b_g:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all()), name
    assert e_l <= b_l, f"{name}: loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    if grad:
        assert e_g <= b_g, f"{name}: grad rel err {e_g:.3e} > {b_g:.3e}"


def frac_l2_above_1(x, gt, sigma, rho, norm):
    from oracle import st as ost
    return float((ost.st_intermediates(x.double(), gt.double(), sigma, rho, norm)["L"][:, 1] > 1).double().mean())


def gs_pointwise_ref(x, gt, sigma, rho, norm, dtype):
    """-> (d, d d.sum() / d S1): autograd of the oracle's pointwise math (normalize, inverse, eigenvalues, distance) on its
    structure tensors in `dtype`."""
    from oracle import st as ost
    S1 = ost.structure_tensor(ost.grayscale(x.to(dtype)), sigma, rho).requires_grad_(True)
    S2 = ost.structure_tensor(ost.grayscale(gt.to(dtype)), sigma, rho)
    d = ost.pixel_distance(S1, S2, norm)
    (g,) = torch.autograd.grad(d.sum(), S1)
    return d.detach(), g.double()


def check_gs(name, x, gt, sigma, rho, norm, gS, loss):
    """gS and the loss straight from a forward entry against gs_pointwise_ref in fp64; yardstick: the same autograd in fp32."""
    (d32, gs32), (d64, gs64) = (gs_pointwise_ref(x, gt, sigma, rho, norm, t) for t in (torch.float32, torch.float64))
    frac = frac_l2_above_1(x, gt, sigma, rho, norm)
    assert frac >= 0.1 and float(gs64.abs().max()) > 0, frac
    e, b = rel_err(gS.cpu(), gs64), truth_bound(gs32, gs64)
    print(f"[{name}] rel err {e:.3e} <= {b:.3e}; loss {loss.item():.6e} vs fp64 {d64.mean().item():.6e}")
    assert bool(torch.isfinite(gS).all())
    assert e <= b, (e, b)
    assert abs(loss.item() - d64.mean().item()) <= max(1e-3 * d64.mean().item(), 3 * abs(d32.double().mean() - d64.mean()).item())


def check_batch_independence(name, x, gt, sigma, rho):
    """Five distinct images: the batched loss is the mean of the five single-image losses, and permuting the batch permutes the
    gradient bit for bit.  (Of the two copies this replaces only the general path's asserted the non-vacuity figure: kept, for both.)"""
    from srganst.loss import StructureTensorLoss
    x[2] = x[2] * 0.5                                  # make the images differ in more than their noise
    gt[4] = gt[4].flip(-1)
    assert frac_l2_above_1(x, gt, sigma, rho, True) >= 0.1
    crit = StructureTensorLoss(sigma, rho)
    lh, gh = loss_hip(x, gt, sigma, rho, True)
    singles = [crit(x[i:i + 1].cuda(), gt[i:i + 1].cuda()).item() for i in range(5)]
    assert len(set(singles)) == 5
    assert abs(lh.item() - np.mean(singles)) <= 1e-6 * abs(lh.item()), (lh.item(), singles)
    perm = torch.tensor([3, 0, 4, 1, 2])
    lp, gp = loss_hip(x[perm].contiguous(), gt[perm].contiguous(), sigma, rho, True)
    assert torch.equal(gp, gh[perm])
    assert abs(lp - lh).item() <= 1e-6 * abs(lh.item())
    check_loss(name, (lh, gh), loss_oracle(x, gt, sigma, rho, True))


def check_non_finite(name, x, gt, xb, gtb, yx, sigma, rho):
    """(xb, gtb) = (x, gt) with one non-finite value at yx of batch entry 1 of 3.  The loss is non-finite exactly when the fp32
    oracle's is (torch.clamp keeps NaN: the clamps must not mask it).  The other images' gradients are bit-identical to a run without
    the bad value.  In the affected image the gradient is non-finite exactly where the oracle's is (the kernel's masked branches
    multiply 0 x NaN as autograd does), and every pixel farther than 2 (R1 + R2) from the bad one (outside its receptive field
    through forward and backward) is bit-identical to the clean run.  (That such pixels exist was asserted by the general path's copy
    only: kept, for both.)"""
    from oracle import st as ost
    R = radius_of(sigma) + radius_of(rho)
    H, W = x.shape[-2:]
    _, gh_clean = loss_hip(x, gt, sigma, rho, True)
    lh, gh = loss_hip(xb, gtb, sigma, rho, True)
    l32, g32 = ost.st_loss_and_grad(xb, gtb, sigma, rho, True)
    print(f"[{name}] loss {lh.item()} (oracle {l32.item()}), non-finite grads hip {int((~torch.isfinite(gh)).sum())} "
          f"oracle {int((~torch.isfinite(g32)).sum())}")
    assert not bool(torch.isfinite(l32))
    assert bool(torch.isfinite(lh)) == bool(torch.isfinite(l32)), (lh.item(), l32.item())
    for b in (0, 2):
        assert torch.equal(gh[b], gh_clean[b]), b
    bad = ~torch.isfinite(g32[1])
    assert bool(bad.any())
    assert torch.equal(~torch.isfinite(gh[1]), bad), "non-finite gradient pattern differs from the oracle's"
    far = torch.ones(H, W, dtype=torch.bool)
    far[max(yx[0] - 2 * R, 0):yx[0] + 2 * R + 1, max(yx[1] - 2 * R, 0):yx[1] + 2 * R + 1] = False
    assert bool(far.any())
    assert torch.equal(gh[1][:, far], gh_clean[1][:, far])
    assert bool(torch.isfinite(g32[1][:, far]).all())


# ------------------------------------------------------------------------------------------------ the maps
def features(S):
    """(t, c2, s2) planes of S [B,3,H,W] in S's dtype: the definition in srganst/st.py."""
    t = S[:, 0] + S[:, 1]
    den = t + 1e-12
    return torch.stack((t, (S[:, 0] - S[:, 1]) / den, 2 * S[:, 2] / den), dim=1)


def maps_oracle(x, gt, sigma, rho, norm, dtype):
    from oracle import st as ost
    it = ost.st_intermediates(x.to(dtype), gt.to(dtype), sigma, rho, norm)
    return {"Sx": it["S1"], "Sgt": it["S2"], "Fx": features(it["S1"]), "Fgt": features(it["S2"]), "d": it["d"], "L": it["L"],
            "distance": it["d"].mean(dim=(1, 2))}


def maps_hip(x, gt, sigma, rho, norm=True, want=ALL):
    from srganst import st
    out = st.st_maps(x.cuda(), None if gt is None else gt.cuda(), sigma, rho, norm, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_distance(name, hip, l32, l64):
    """The loss rule, per image."""
    for b in range(l64.numel()):
        e, bound = abs(hip[b].item() - l64[b].item()), max(1e-3 * abs(l64[b].item()), 3 * abs(l32[b].item() - l64[b].item()))
        print(f"[{name}] image {b}: distance {hip[b].item():.6e} |hip-l64| {e:.3e} <= {bound:.3e}")
        assert math.isfinite(hip[b].item()) and e <= bound, (name, b, hip[b].item(), l64[b].item(), e, bound)


def check_maps_vs_fp64(name, x, gt, sigma, rho, norm, min_trace):
    """Every map and the per-image distances of one st_maps call under the truth rule -> the call's outputs.  Not vacuous: l2 > 1 on
    a tenth of the pixels, and the trace stays above min_trace, where the 1e-12 guard of the features takes no part (the callers
    keep their own: 5e-4 on the tile builds; 1.7e-5 = 1e-12 / 2^-24, half an fp32 ulp, on the general path, whose wider kernels
    smooth the trace down to 1.7e-4 on its inputs)."""
    B, _, H, W = x.shape
    o32, o64 = maps_oracle(x, gt, sigma, rho, norm, torch.float32), maps_oracle(x, gt, sigma, rho, norm, torch.float64)
    frac = float((o64["L"][:, 1] > 1).double().mean())
    assert frac >= 0.1, f"vacuous case: only {frac:.1%} of the pixels have l2 > 1"
    trace = min(float(o64["Fx"][:, 0].min()), float(o64["Fgt"][:, 0].min()))
    assert trace >= min_trace, f"trace {trace:.3e}: the 1e-12 guard of the features would take part"
    got = maps_hip(x, gt, sigma, rho, norm)
    for key in ("Sx", "Sgt", "d", "Fx", "Fgt"):
        assert got[key].dtype == torch.float32 and got[key].shape == o64[key].shape, (key, got[key].shape)
        assert bool(torch.isfinite(got[key]).all()), key
        e, b = rel_err(got[key], o64[key]), truth_bound(o32[key], o64[key])
        print(f"[{name}] {key}: rel err {e:.3e} <= {b:.3e}")
        assert e <= b, f"{name} {key}: rel err {e:.3e} > {b:.3e}"
    tiles = ((H + 31) // 32) * ((W + 31) // 32)
    assert tuple(got["tile_sums"].shape) == (B, tiles) and got["distance"].dtype == torch.float64
    check_distance(name, got["distance"], o32["distance"].double(), o64["distance"])
    return got


def check_optional_outputs_are_the_same_bits(x, gt, sigma, rho):
    full = maps_hip(x, gt, sigma, rho)
    for key in ALL:
        alone = maps_hip(x, gt, sigma, rho, want=(key,))
        assert list(alone) == [key]
        assert torch.equal(alone[key], full[key]), f"{key} requested alone differs from the all-outputs call"
    x_only = maps_hip(x, None, sigma, rho, want=("Sx", "Fx"))
    assert torch.equal(x_only["Sx"], full["Sx"]) and torch.equal(x_only["Fx"], full["Fx"])
    swapped = maps_hip(gt, x, sigma, rho, want=("Sx", "Sgt"))              # both images run the same code
    assert torch.equal(swapped["Sx"], full["Sgt"]) and torch.equal(swapped["Sgt"], full["Sx"])
