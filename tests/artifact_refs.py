"""The contract of ArtifactLoss (the artifact-map / locally discriminative loss of Liang et al., CVPR 2022) restated in plain torch
(dtype-generic: pad, unfold, var): what csrc/artifact_loss.hip is held to.  sr, gt and the optional ref are [B,3,H,W], k = ksize
is odd, p = k // 2:

    r, r_e   sum over R, G, B (added in that order) of |gt - sr| and of |gt - ref|                              [B,1,H,W]
    s_b      (the unbiased variance of r over the H*W pixels of image b) ** (1/5)                               the global weight
    v        the unbiased variance (divisor k*k - 1) of the k x k window of r, r reflect-padded by p            the local weight
    w        s_b * v, and 0 where r < r_e strictly (only with ref): ref == sr masks nothing
    loss     mean over B*3*H*W of w * |sr - gt|; w is a constant of the gradient, so d loss / d sr = w sign(sr - gt) / (3 B H W)
    the gradient is taken with respect to sr only.

Also the shared inputs of tests/test_artifact_refs.py and tests/test_artifact_loss_gpu.py: gt = rand, sr = gt + 0.1 randn, ref = gt +
0.1 randn; each case's images and its fp32 / fp64 results are computed once and never modified.  The seeds keep two conditions that
tests/test_artifact_refs.py asserts for every case: the masked share of the pixels lies in [0.25, 0.75], and min |r - r_e| >= 1e-6
in fp64, so no mask decision depends on the precision."""
import functools

import torch
import torch.nn.functional as F

# name -> (seed, B, H, W, ksize): see tests/test_artifact_loss_gpu.py for why each is there
CASES = {"tiny": (1, 1, 4, 4, 7), "seams": (1, 2, 33, 65, 7), "ragged": (1, 1, 75, 64, 7), "k3": (1, 2, 19, 43, 3),
         "k11": (1, 2, 19, 43, 11), "medium": (1, 2, 48, 40, 7)}


def images(seed, B, H, W):
    """-> (sr, gt, ref), fp32."""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, 3, H, W, generator=gen)
    sr = gt + 0.1 * torch.randn(B, 3, H, W, generator=gen)
    ref = gt + 0.1 * torch.randn(B, 3, H, W, generator=gen)
    return sr, gt, ref


def residual(x, gt):
    """sum over R, G, B of |gt - x|, added in that order -> [B,1,H,W]."""
    d = (gt - x).abs()
    return (d[:, 0:1] + d[:, 1:2]) + d[:, 2:3]


def global_weight(r):
    """s_b [B] of r [B,1,H,W]."""
    return r.reshape(r.shape[0], -1).var(dim=1, unbiased=True) ** (1 / 5)


def local_variance(r, ksize=7):
    """v [B,1,H,W]: the unbiased variance of every k x k window of the reflect-padded r."""
    B, _, H, W = r.shape
    p = ksize // 2
    windows = F.unfold(F.pad(r, (p, p, p, p), mode="reflect"), ksize)          # [B, k*k, H*W]
    return windows.var(dim=1, unbiased=True).reshape(B, 1, H, W)


def mask(sr, gt, ref):
    """True where the map is switched off: sr is strictly closer to gt than ref is."""
    return residual(sr, gt) < residual(ref, gt)


def weight_map(sr, gt, ref=None, ksize=7):
    """w [B,1,H,W]; no graph is built through it."""
    with torch.no_grad():
        r = residual(sr, gt)
        w = global_weight(r).view(-1, 1, 1, 1) * local_variance(r, ksize)
        if ref is not None:
            w = torch.where(r < residual(ref, gt), torch.zeros_like(w), w)
    return w


def artifact_loss(sr, gt, ref=None, ksize=7):
    return (weight_map(sr, gt, ref, ksize) * (sr - gt).abs()).mean()


def analytic_grad(sr, gt, ref=None, ksize=7):
    """d loss / d sr as the contract states it: w sign(sr - gt) / (3 B H W), sign(0) = 0."""
    return weight_map(sr, gt, ref, ksize) * torch.sign(sr - gt) / sr.numel()


def loop_loss(sr, gt, ref=None, ksize=7):
    """The same loss with Python loops over fp64 scalars - for one tiny case.  -> (loss, w as nested lists [B][H][W])."""
    B, _, H, W = sr.shape
    p, n = ksize // 2, ksize * ksize
    s, g = sr.double().tolist(), gt.double().tolist()
    e = ref.double().tolist() if ref is not None else None

    def res(a, b, y, x):
        return (abs(g[b][0][y][x] - a[b][0][y][x]) + abs(g[b][1][y][x] - a[b][1][y][x])) + abs(g[b][2][y][x] - a[b][2][y][x])

    def refl(i, size):
        return -i if i < 0 else 2 * (size - 1) - i if i >= size else i

    total, maps = 0.0, []
    for b in range(B):
        r = [[res(s, b, y, x) for x in range(W)] for y in range(H)]
        flat = [v for row in r for v in row]
        mean = sum(flat) / len(flat)
        sb = (sum((v - mean) ** 2 for v in flat) / (len(flat) - 1)) ** (1 / 5)
        wb = [[0.0] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                win = [r[refl(y + dy, H)][refl(x + dx, W)] for dy in range(-p, p + 1) for dx in range(-p, p + 1)]
                m = sum(win) / n
                w = sb * (sum((v - m) ** 2 for v in win) / (n - 1))
                if e is not None and r[y][x] < res(e, b, y, x):
                    w = 0.0
                wb[y][x] = w
                total += w * r[y][x]
        maps.append(wb)
    return total / (B * 3 * H * W), maps


def loss_and_grad(sr, gt, ref, ksize, dtype=torch.float64):
    """The restatement evaluated in `dtype` -> (loss, d loss / d sr by autograd), both as fp64 tensors."""
    x = sr.detach().clone().to(dtype).requires_grad_(True)                # a copy: sr itself stays a plain tensor
    l = artifact_loss(x, gt.to(dtype), None if ref is None else ref.to(dtype), ksize)
    (g,) = torch.autograd.grad(l, x)
    return l.detach().double(), g.double()


@functools.lru_cache(maxsize=None)
def case(name, with_ref=True):
    """-> (sr, gt, ref or None, l32, g32, l64, g64) of one table case: the fp32 and the fp64 evaluation of the restatement."""
    seed, B, H, W, k = CASES[name]
    sr, gt, ref = images(seed, B, H, W)
    ref = ref if with_ref else None
    return (sr, gt, ref, *loss_and_grad(sr, gt, ref, k, torch.float32), *loss_and_grad(sr, gt, ref, k, torch.float64))


def mask_facts(name):
    """(the masked share of the pixels, min |r - r_e|) of a case in fp64."""
    seed, B, H, W, _ = CASES[name]
    sr, gt, ref = (t.double() for t in images(seed, B, H, W))
    r, re = residual(sr, gt), residual(ref, gt)
    return float((r < re).double().mean()), float((r - re).abs().min())
