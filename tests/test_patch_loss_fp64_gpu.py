"""The best-buddy patch losses (BestBuddyLoss, GramLoss, PatchwiseStructureTensorLoss; csrc/bb_loss.hip) on the GPU against
an fp64 restatement of the same operation evaluated AT THE KERNEL'S OWN MATCHES (oracle/bb.py, ind=).

The reference fixtures (tests/test_bestbuddy.py) can only hold the HIP path loosely: buddy choices that tie within fp32 noise may
go either way, and one flipped buddy moves the loss and the gradient by the difference of two near-equal candidates.  Here the
discrete choice and the arithmetic are checked apart:
  - selection: the HIP's pick is a valid argmin of the fp64 score - its slack (score64[i, pick] - min_j score64[i, j]) stays within
    tau_i = 3 x the fp32 oracle's own rounding on row i (the larger of its pick's slack and twice its largest score error on the
    row) + 4 ulp of the row minimum; where the fp64 runner-up is farther than tau_i the pick is the fp64 argmin itself;
  - loss and gradient at the HIP's picks: within max(1e-5, 3 x the fp32 oracle's distance from fp64 at the same picks).
Non-finite inputs: the matcher follows torch.min (NaN is the minimum, the first NaN / the first minimum wins) and no index can
leave the candidate table.  Capture: a patch loss inside TrainEngine's captured iteration reproduces the eager run bit for bit."""
import zlib

import pytest
import torch

from conftest import rel_err
from graph_refs import graph_vs_eager

pytestmark = pytest.mark.gpu


U32 = 2.0 ** -24                 # fp32 unit roundoff
ALPHA_BETA = {"a1b1": (1.0, 1.0), "a05b2": (0.5, 2.0), "a0b1": (0.0, 1.0)}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 10000           # stable across processes (str hashes are salted)


def _images(seed, B, H, W):
    """B independent smooth images (bicubic-upsampled noise + fine noise, on the 1/255 grid) and an SR estimate near each."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(2, H // 4), max(2, W // 4), generator=gen)
    gt = F.interpolate(base, size=(H, W), mode="bicubic", align_corners=False) + 0.05 * torch.randn(B, 3, H, W, generator=gen)
    gt = torch.round(gt.clamp(0, 1) * 255) / 255
    x = (gt + 0.08 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    return x, gt


def _saturated(seed, B, H, W):
    """GT with 12 x 12 blocks (aligned with the 3 x 3 patches at every scale) of exact 0 and exact 1; SR equals GT on them."""
    x, gt = _images(seed, B, H, W)
    for b in range(B):
        for k, (y0, x0) in enumerate(((0, 0), (12, 24), (24, 12), (H - 12, W - 12))):
            v = float((k + b) % 2)
            gt[b, :, y0:y0 + 12, x0:x0 + 12] = v
            x[b, :, y0:y0 + 12, x0:x0 + 12] = v
    return x, gt


def _module(kind, alpha, beta, dist, crit, geom=(3, 0, 3)):
    from srganst.loss import BestBuddyLoss, GramLoss, PatchwiseStructureTensorLoss
    if kind == "bb":
        k, pad, stride = geom
        return BestBuddyLoss(alpha=alpha, beta=beta, ksize=k, pad=pad, stride=stride, dist_norm=dist, criterion=crit)
    cls = GramLoss if kind == "gram" else PatchwiseStructureTensorLoss
    return cls(alpha=alpha, beta=beta, dist_norm=dist, criterion=crit)


def _oracle(kind, x, gt, alpha, beta, dist, crit, geom=(3, 0, 3), ind=None):
    """-> (loss, d loss / d x, score, SR features [B, np, D], candidate table [B, ncand, D]) of oracle/bb.py in x's dtype."""
    import torch.nn.functional as F
    from oracle import bb
    x = x.detach().clone().requires_grad_(True)
    if kind == "bb":
        k, pad, stride = geom
        loss, _, score = bb.best_buddy_loss(x, gt, alpha, beta, k, pad, stride, dist, crit, ind=ind)
        p1, cat = bb.patches(x.detach(), k, pad, stride), bb.candidates(gt, k, pad, stride)[0]
    else:
        fn, fe = (bb.gram_loss, bb.gram_patches) if kind == "gram" else (bb.patchwise_st_loss, bb.st_patches)
        loss, _, score = fn(x, gt, alpha=alpha, beta=beta, dist_norm=dist, criterion=crit, ind=ind)
        gt2 = F.interpolate(gt, scale_factor=0.5, mode="bicubic", align_corners=False)
        gt4 = F.interpolate(gt, scale_factor=0.25, mode="bicubic", align_corners=False)
        p1, cat = fe(x.detach()), torch.cat([fe(gt), fe(gt2), fe(gt4)], 1)
    (gx,) = torch.autograd.grad(loss, x)
    return loss.detach(), gx, score.detach(), p1, cat


def _check_selection(ind, score64, score32, rows=None):
    """The HIP's picks `ind` [B, np] against the fp64 score.  tau (per row) = 3 x the fp32 oracle's own rounding on that row: the
    larger of its pick's fp64 slack and twice its largest score error, plus 4 ulp of the row's smallest score.  -> max slack / tau."""
    ind = ind.long()
    ncand = score64.shape[2]
    assert int(ind.min()) >= 0 and int(ind.max()) < ncand
    smin64, amin64 = torch.min(score64, dim=2)
    top2 = torch.topk(score64, min(2, ncand), dim=2, largest=False).values
    margin = top2[..., 1] - top2[..., 0] if ncand > 1 else torch.full_like(smin64, float("inf"))
    ind32 = torch.min(score32, dim=2)[1]
    slack32 = torch.gather(score64, 2, ind32.unsqueeze(-1)).squeeze(-1) - smin64
    err32 = (score32.double() - score64).abs().amax(dim=2)
    tau = 3.0 * torch.maximum(slack32, 2.0 * err32) + 4 * U32 * smin64.abs()
    slack = torch.gather(score64, 2, ind.unsqueeze(-1)).squeeze(-1) - smin64
    if rows is None:
        rows = torch.ones_like(slack, dtype=torch.bool)
    assert bool((slack[rows] <= tau[rows]).all()), f"pick off the fp64 argmin by {float((slack - tau)[rows].max()):.3e} beyond tau"
    clear = rows & (margin > tau)
    assert torch.equal(ind[clear], amin64[clear]), "a pick differs from the fp64 argmin where the runner-up is clear of rounding"
    ratio = float((slack[rows] / tau[rows].clamp_min(1e-300)).max()) if bool(rows.any()) else 0.0
    return ratio, float(clear[rows].float().mean()) if bool(rows.any()) else 1.0


def _pixel_mask(row_mask, H, W, geom):
    """Pixels not touched by any patch flagged in row_mask [B, np] (F.unfold's adjoint of the flags)."""
    import torch.nn.functional as F
    k, pad, stride = geom
    B = row_mask.shape[0]
    flags = row_mask.double().unsqueeze(1).expand(B, 3 * k * k, -1)
    return F.fold(flags, (H, W), kernel_size=k, padding=pad, stride=stride) == 0


def _run_case(kind, x, gt, alpha, beta, dist, crit, geom=(3, 0, 3), label=""):
    mod = _module(kind, alpha, beta, dist, crit, geom)
    xg = x.cuda().requires_grad_(True)
    loss = mod(xg, gt.cuda())
    (g_hip,) = torch.autograd.grad(loss, xg)
    ind = mod.last_index.cpu().long()
    loss_hip, g_hip = float(loss), g_hip.cpu().double()
    l64, g64, s64, p64, c64 = _oracle(kind, x.double(), gt.double(), alpha, beta, dist, crit, geom, ind=ind)
    l32, g32, s32, p32, c32 = _oracle(kind, x, gt, alpha, beta, dist, crit, geom, ind=ind)
    ratio, clear = _check_selection(ind, s64, s32)
    # loss at the HIP's picks
    e_loss, b_loss = abs(loss_hip - float(l64)) / abs(float(l64)), max(1e-5, 3 * abs(float(l32) - float(l64)) / abs(float(l64)))
    assert e_loss <= b_loss, f"{label} loss: {e_loss:.3e} > {b_loss:.3e}"
    # gradient at the HIP's picks; L1 criterion: features whose fp64 difference is nonzero but below fp32 rounding may take either
    # sign - the pixels of their patches are left out (exact zeros are not: sign(0) = 0 must come out)
    nmask = 0
    keep = torch.ones_like(g64, dtype=torch.bool)
    if crit == "l1":
        sel = lambda c, p: torch.gather(c, 1, ind.unsqueeze(-1).expand(-1, -1, p.shape[2]))
        df64, df32 = p64 - sel(c64, p64), p32 - sel(c32, p32)
        delta = 3 * (df32.double() - df64).abs().max()
        small = (df64 != 0) & (df64.abs() < delta)
        nmask = int(small.sum())
        keep = _pixel_mask(small.any(dim=2), x.shape[2], x.shape[3], geom)
    g64m = torch.where(keep, g64, torch.zeros_like(g64))
    e_grad = rel_err(torch.where(keep, g_hip, torch.zeros_like(g_hip)), g64m)
    b_grad = max(1e-5, 3 * rel_err(torch.where(keep, g32.double(), torch.zeros_like(g64)), g64m))
    print(f"[{label}] slack/tau max {ratio:.3f} (clear rows {clear:.3f}); loss err {e_loss:.2e} (bound {b_loss:.2e}); "
          f"grad err {e_grad:.2e} (bound {b_grad:.2e}); masked features {nmask}")
    assert e_grad <= b_grad, f"{label} grad: {e_grad:.3e} > {b_grad:.3e}"
    zero = keep & (g64 == 0)
    assert bool((g_hip[zero] == 0).all()), f"{label}: {int((g_hip[zero] != 0).sum())} gradient entries nonzero where the fp64 one is 0"
    return ind


# kind, (H, W), dist, crit, alpha/beta
DEFAULT_CASES = [(kind, hw, dist, crit, "a1b1") for kind in ("bb", "gram", "pst") for hw in ((48, 48),) for dist in ("l2", "l1")
                 for crit in ("l1", "l2")]
DEFAULT_CASES += [(kind, (36, 60), dist, "l1", "a05b2") for kind in ("bb", "gram", "pst") for dist in ("l2", "l1")]
DEFAULT_CASES += [(kind, (48, 48), "l2", "l1", "a0b1") for kind in ("bb", "gram", "pst")]
DEFAULT_CASES += [(kind, (96, 96), "l2", crit, "a1b1") for kind in ("bb", "gram", "pst") for crit in ("l1", "l2")]
DEFAULT_CASES += [(kind, (36, 60), "l1", "l2", "a0b1") for kind in ("gram", "pst")]
DEFAULT_CASES += [(kind, (192, 192), "l2", "l1", "a1b1") for kind in ("bb", "gram", "pst")]


@pytest.mark.parametrize("kind,hw,dist,crit,ab", DEFAULT_CASES,
                         ids=[f"{k}-{h}x{w}-d{d}-c{c}-{ab}" for k, (h, w), d, c, ab in DEFAULT_CASES])
def test_patch_loss_default_path_vs_fp64(kind, hw, dist, crit, ab):
    """The register-resident kernels (bb_patches_kernel + bb_match_kernel; H, W multiples of 12), B = 3 independent images: 36 x 60
    has 240 patches (a partial 32-query workgroup), 192 x 192 is the HR crop size."""
    x, gt = _images(_seed(kind, hw, dist, crit, ab), 3, *hw)
    _run_case(kind, x, gt, *ALPHA_BETA[ab], dist, crit, label=f"{kind} {hw} {dist}/{crit} {ab}")


# (H, W), (ksize, pad, stride)
GENERAL_CASES = [((45, 42), (3, 0, 3)), ((4, 4), (3, 1, 3)), ((24, 30), (3, 1, 2))]


@pytest.mark.parametrize("dist", ["l2", "l1"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("hw,geom", GENERAL_CASES, ids=["45x42-k3p0s3", "4x4-k3p1s3", "24x30-k3p1s2"])
def test_best_buddy_general_path_vs_fp64(hw, geom, crit, dist):
    """The table-based kernels (bbg_*): odd non-square images (268 candidates), a 4 x 4 image with 6 candidates (fewer than the
    8 candidate splits) and overlapping patches (the gradient is the unfold's adjoint)."""
    x, gt = _images(_seed(hw, geom, crit, dist), 3, *hw)
    _run_case("bb", x, gt, 1.0, 1.0, dist, crit, geom, label=f"bb {hw} {geom} {dist}/{crit}")


@pytest.mark.parametrize("dist", ["l2", "l1"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("kind", ["bb", "gram", "pst", "bb-general"])
def test_patch_loss_saturated_regions_vs_fp64(kind, crit, dist):
    """SR == GT on blocks of exact 0 and exact 1: the candidate features the match kernel computes for the SR patch must equal the
    table's (bb_patches_kernel) bit for bit, or the L1 criterion's sign(0) turns into +-1 where the reference's gradient is 0."""
    general = kind == "bb-general"
    hw = (45, 42) if general else (48, 48)
    x, gt = _saturated(_seed(kind, crit, dist), 3, *hw)
    _run_case("bb" if general else kind, x, gt, 1.0, 1.0, dist, crit, label=f"saturated {kind} {dist}/{crit}")


@pytest.mark.parametrize("dist", ["l2", "l1"])
@pytest.mark.parametrize("where", ["sr-nan", "sr-posinf", "sr-neginf", "gt-nan"])
@pytest.mark.parametrize("kind", ["bb", "gram", "pst", "bb-general"])
def test_patch_loss_non_finite_inputs_follow_torch_min(kind, where, dist):
    """A NaN / +inf / -inf in one SR patch, or a NaN in one GT patch: the matcher follows torch.min (a NaN score is the minimum, the
    first NaN / first minimum wins), the L2 distance's clamp keeps NaN like torch.clamp, no index leaves [0, ncand), and the loss is
    non-finite exactly when the fp32 oracle's is."""
    general = kind == "bb-general"
    kind = "bb" if general else kind
    hw = (45, 42) if general else (48, 48)
    x, gt = _images(_seed(kind, where, dist, general), 3, *hw)
    v = {"nan": float("nan"), "posinf": float("inf"), "neginf": float("-inf")}[where.split("-")[1]]
    (x if where.startswith("sr") else gt)[1, 1, 13, 7] = v                       # batch entry 1, patch (4, 2), pixel (1, 1), channel 1
    mod = _module(kind, 1.0, 1.0, dist, "l1")
    loss = mod(x.cuda(), gt.cuda())
    torch.cuda.synchronize()
    ind = mod.last_index.cpu().long()
    l32, _, s32, _, _ = _oracle(kind, x, gt, 1.0, 1.0, dist, "l1")
    ncand = s32.shape[2]
    assert int(ind.min()) >= 0 and int(ind.max()) < ncand
    assert bool(torch.isfinite(loss).item()) == bool(torch.isfinite(l32).item()), (float(loss), float(l32))
    nonfinite = ~torch.isfinite(s32).all(dim=2)
    assert bool(nonfinite.any())
    ind32 = torch.min(s32, dim=2)[1]
    assert torch.equal(ind[nonfinite], ind32[nonfinite]), (ind[nonfinite], ind32[nonfinite])
    rows = ~nonfinite
    if bool(rows.any()):
        _, _, s64, _, _ = _oracle(kind, x.double(), gt.double(), 1.0, 1.0, dist, "l1")
        ok64 = torch.isfinite(s64).all(dim=2)
        _check_selection(torch.where(rows & ok64, ind, torch.zeros_like(ind)), s64.nan_to_num(), s32.nan_to_num(), rows & ok64)
    print(f"[{kind}{' general' if general else ''} {where} {dist}] loss {float(loss)} (oracle {float(l32)}), "
          f"{int(nonfinite.sum())} non-finite rows")


@pytest.mark.parametrize("schedule", ["shared", "batched"])
@pytest.mark.parametrize("loss", ["BestBuddy", "Gram", "PatchwiseST-l2", "PatchwiseST-l1"])
def test_train_engine_graph_equals_eager_with_patch_loss(loss, schedule):
    """Adversarial + Pixel + ST + one patch loss at its reference weight (MODEL.G_LOSS.CRITERION_WEIGHTS) through TrainEngine:
    the captured two-branch iteration (the criteria run inside it, engine._criterion_total) equals the eager one bit for bit over
    5 iterations.  schedule 'shared': the discriminator step reuses the generator step's D(sr) pass (KERNEL.REUSE_D_SR, the
    default); 'batched': D(gt) and D(sr.detach()) run as one batch (KERNEL.BATCH_D_STEP)."""
    from srganst.loss import BestBuddyLoss, GramLoss, PatchwiseStructureTensorLoss
    name, _, dist = loss.partition("-")
    cls = {"BestBuddy": BestBuddyLoss, "Gram": GramLoss, "PatchwiseST": PatchwiseStructureTensorLoss}[name]
    graph_vs_eager(lambda cfg: [(name, cls(dist_norm=dist or "l2"))], schedule == "shared")
