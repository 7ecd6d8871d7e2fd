"""BestBuddyLoss: the CPU oracle against the reference's own outputs (tests/golden/bestbuddy_<case>.npz, generated
by make_golden_bb.py from loss.py:78-142), and the HIP path against both."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err

G = {name: os.path.join(os.path.dirname(__file__), "golden", f"bestbuddy_{name}.npz") for name in ("lf48", "lf96")}   # one file per case


@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_oracle_matches_reference_golden(name, crit):
    from oracle import bb
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"])
    loss, ind, _ = bb.best_buddy_loss(x, gt, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert torch.equal(loss.detach(), torch.from_numpy(g[f"{name}/{crit}/loss"]))
    assert torch.equal(gx, torch.from_numpy(g[f"{name}/{crit}/grad"]))
    assert np.array_equal(ind.numpy(), g[f"{name}/ind"])
    cat, gt2, gt4 = bb.candidates(gt)
    assert torch.equal(gt2, torch.from_numpy(g[f"{name}/gt2"])) and torch.equal(gt4, torch.from_numpy(g[f"{name}/gt4"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_hip_best_buddy_matches_reference_golden(name, crit):
    from srganst.loss import BestBuddyLoss
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"]).cuda()
    mod = BestBuddyLoss(criterion=crit)
    loss = mod(x, gt)
    (gx,) = torch.autograd.grad(loss * 2.0, x)
    ref_loss = float(g[f"{name}/{crit}/loss"])
    assert abs(loss.item() - ref_loss) < 1e-5 * abs(ref_loss)
    # every selected buddy equals the reference's wherever the runner-up is not within fp32 noise of the winner
    ind, margin = mod.last_index.cpu().numpy(), g[f"{name}/margin"]
    clear = margin > 1e-4
    assert clear.mean() > 0.99 and np.array_equal(ind[clear], g[f"{name}/ind"][clear])
    assert rel_err(gx.cpu() * 0.5, torch.from_numpy(g[f"{name}/{crit}/grad"])) < (1e-6 if clear.all() else 1e-2)


@pytest.mark.gpu
def test_hip_best_buddy_vs_oracle_hard_matching():
    """Unrelated SR / GT images: the best buddy is NOT the co-located patch, multi-scale candidates matter."""
    from oracle import bb
    from srganst.loss import BestBuddyLoss
    g = torch.Generator().manual_seed(17)
    gt = torch.rand(2, 3, 48, 48, generator=g)
    x = torch.rand(2, 3, 48, 48, generator=g).requires_grad_(True)
    loss_o, ind_o, score = bb.best_buddy_loss(x, gt, alpha=1.0, beta=0.5)
    (g_o,) = torch.autograd.grad(loss_o, x)
    top2 = torch.topk(score, 2, dim=2, largest=False).values
    clear = ((top2[..., 1] - top2[..., 0]) > 1e-4).numpy()
    mod = BestBuddyLoss(alpha=1.0, beta=0.5)
    xg = x.detach().cuda().requires_grad_(True)
    loss = mod(xg, gt.cuda())
    loss.backward()
    ind = mod.last_index.cpu().numpy()
    assert clear.mean() > 0.95 and np.array_equal(ind[clear], ind_o.numpy()[clear])
    assert (ind_o.numpy() >= 256).any()                     # some buddies come from the 1/2 or 1/4 scale
    assert abs(loss.item() - loss_o.item()) < 1e-3 * abs(loss_o.item())
    assert rel_err(xg.grad.cpu(), g_o) < 2e-2                # a near-tie flips the sign pattern of one patch


@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_gram_oracle_matches_reference_golden(name, crit):
    from oracle import bb
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"])
    assert torch.equal(bb.gram_patches(x.detach()), torch.from_numpy(g[f"{name}/gram/p1"]))
    loss, ind, _ = bb.gram_loss(x, gt, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert torch.equal(loss.detach(), torch.from_numpy(g[f"{name}/gram/{crit}/loss"]))
    assert torch.equal(gx, torch.from_numpy(g[f"{name}/gram/{crit}/grad"]))
    assert np.array_equal(ind.numpy(), g[f"{name}/gram/ind"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_hip_gram_loss_matches_reference_golden(name, crit):
    """Gram features are 4th-order in the pixels and many candidates are near-ties: buddies are compared where the reference's
    margin is clear of fp32 noise, the loss with the tolerance that the remaining flips allow."""
    from srganst.loss import GramLoss
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"]).cuda()
    mod = GramLoss(criterion=crit)
    loss = mod(x, gt)
    (gx,) = torch.autograd.grad(loss, x)
    ind, margin = mod.last_index.cpu().numpy(), g[f"{name}/gram/margin"]
    clear = margin > 2e-6
    assert clear.mean() > 0.97 and np.array_equal(ind[clear], g[f"{name}/gram/ind"][clear])
    ref_loss = float(g[f"{name}/gram/{crit}/loss"])
    assert abs(loss.item() - ref_loss) < 1e-3 * abs(ref_loss)
    assert rel_err(gx.cpu(), torch.from_numpy(g[f"{name}/gram/{crit}/grad"])) < 5e-2


@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_patchwise_st_oracle_matches_reference_golden(name, crit):
    from oracle import bb
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"])
    assert torch.equal(bb.st_patches(x.detach()), torch.from_numpy(g[f"{name}/pst/p1"]))
    loss, ind, _ = bb.patchwise_st_loss(x, gt, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert torch.equal(loss.detach(), torch.from_numpy(g[f"{name}/pst/{crit}/loss"]))
    assert rel_err(gx, torch.from_numpy(g[f"{name}/pst/{crit}/grad"])) < 1e-6
    assert np.array_equal(ind.numpy(), g[f"{name}/pst/ind"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lf48", "lf96"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_hip_patchwise_st_matches_reference_golden(name, crit):
    from srganst.loss import PatchwiseStructureTensorLoss
    g = np.load(G[name])
    x = torch.from_numpy(g[f"{name}/x"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"]).cuda()
    mod = PatchwiseStructureTensorLoss(criterion=crit)
    loss = mod(x, gt)
    (gx,) = torch.autograd.grad(loss, x)
    ind, margin = mod.last_index.cpu().numpy(), g[f"{name}/pst/margin"]
    clear = margin > 2e-5
    assert clear.mean() > 0.97 and np.array_equal(ind[clear], g[f"{name}/pst/ind"][clear])
    ref_loss = float(g[f"{name}/pst/{crit}/loss"])
    assert abs(loss.item() - ref_loss) < 1e-3 * abs(ref_loss)
    assert rel_err(gx.cpu(), torch.from_numpy(g[f"{name}/pst/{crit}/grad"])) < 5e-2


# ---- off the reference's default configuration: other patch geometries and the L1 matching distance (tests/golden/bestbuddy_geom.npz,
# generated by make_golden_bb_geom.py from the reference itself)
GG = os.path.join(os.path.dirname(__file__), "golden", "bestbuddy_geom.npz")
BB_CASES = {"k3p1s2_l2": (3, 1, 2, "l2", "l1"), "k5p0s5_l1": (5, 0, 5, "l1", "l2"), "k3p0s3_l1": (3, 0, 3, "l1", "l1"),
            "k4p2s3_l2": (4, 2, 3, "l2", "l2")}


@pytest.mark.parametrize("name", list(BB_CASES))
def test_oracle_general_geometry_matches_reference_golden(name):
    from oracle import bb
    k, pad, stride, dn, crit = BB_CASES[name]
    g = np.load(GG)
    x = torch.from_numpy(g[f"bb/{name}/x"]).requires_grad_(True)
    gt = torch.from_numpy(g[f"bb/{name}/gt"])
    loss, ind, _ = bb.best_buddy_loss(x, gt, ksize=k, pad=pad, stride=stride, dist_norm=dn, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert torch.equal(loss.detach(), torch.from_numpy(g[f"bb/{name}/loss"]))
    assert torch.equal(gx, torch.from_numpy(g[f"bb/{name}/grad"]))
    assert np.array_equal(ind.numpy(), g[f"bb/{name}/ind"])


@pytest.mark.parametrize("tag", ["gram", "pst"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_oracle_l1_distance_matches_reference_golden(tag, crit):
    from oracle import bb
    g = np.load(GG)
    x = torch.from_numpy(g["l1/x"]).requires_grad_(True)
    gt = torch.from_numpy(g["l1/gt"])
    fn = bb.gram_loss if tag == "gram" else bb.patchwise_st_loss
    loss, ind, _ = fn(x, gt, dist_norm="l1", criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert abs(float(loss) - float(g[f"l1/{tag}/{crit}/loss"])) <= 1e-6 * abs(float(g[f"l1/{tag}/{crit}/loss"]))
    assert rel_err(gx, torch.from_numpy(g[f"l1/{tag}/{crit}/grad"])) < 1e-5
    clear = g[f"l1/{tag}/margin"] > 0          # exact ties (flat patches have identical features): topk's pick is not torch.min's
    assert clear.mean() > 0.75 and np.array_equal(ind.numpy()[clear], g[f"l1/{tag}/ind"][clear])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BB_CASES))
def test_hip_best_buddy_general_geometry_matches_reference_golden(name):
    """ksize / pad / stride / dist_norm off the defaults (reference loss.py:86): table-based kernels (overlapping patches: the
    gradient is the unfold's adjoint), or - default geometry with the L1 distance - the register-resident ones."""
    from srganst.loss import BestBuddyLoss
    k, pad, stride, dn, crit = BB_CASES[name]
    g = np.load(GG)
    x = torch.from_numpy(g[f"bb/{name}/x"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g[f"bb/{name}/gt"]).cuda()
    mod = BestBuddyLoss(ksize=k, pad=pad, stride=stride, dist_norm=dn, criterion=crit)
    loss = mod(x, gt)
    (gx,) = torch.autograd.grad(loss * 2.0, x)
    ref_loss = float(g[f"bb/{name}/loss"])
    ind, margin = mod.last_index.cpu().numpy(), g[f"bb/{name}/margin"]
    clear = margin > 1e-4 * max(1.0, float(g[f"bb/{name}/score_scale"]))
    assert clear.mean() > 0.97 and np.array_equal(ind[clear], g[f"bb/{name}/ind"][clear])
    assert abs(loss.item() - ref_loss) < (1e-5 if clear.all() else 1e-3) * abs(ref_loss)
    assert rel_err(gx.cpu() * 0.5, torch.from_numpy(g[f"bb/{name}/grad"])) < (1e-6 if clear.all() else 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["gram", "pst"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_hip_gram_and_patchwise_st_l1_distance(tag, crit):
    from srganst.loss import GramLoss, PatchwiseStructureTensorLoss
    g = np.load(GG)
    x = torch.from_numpy(g["l1/x"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g["l1/gt"]).cuda()
    mod = (GramLoss if tag == "gram" else PatchwiseStructureTensorLoss)(dist_norm="l1", criterion=crit)
    loss = mod(x, gt)
    (gx,) = torch.autograd.grad(loss, x)
    ref_loss = float(g[f"l1/{tag}/{crit}/loss"])
    ind, margin = mod.last_index.cpu().numpy(), g[f"l1/{tag}/margin"]
    clear = margin > 1e-4                      # (18 % of the structure-tensor features tie exactly: flat patches)
    assert clear.mean() > 0.75 and np.array_equal(ind[clear], g[f"l1/{tag}/ind"][clear])
    # patches whose runner-up is within fp32 noise of the winner may pick the other buddy (the structure-tensor features carry
    # 1 / sqrt(det + 1e-12): near-flat patches amplify rounding), which moves the loss by the difference of two near-equal candidates
    assert abs(loss.item() - ref_loss) < (2e-3 if tag == "gram" else 5e-2) * abs(ref_loss)
    assert rel_err(gx.cpu(), torch.from_numpy(g[f"l1/{tag}/{crit}/grad"])) < (5e-2 if tag == "gram" else 0.5)


@pytest.mark.gpu
def test_hip_best_buddy_general_path_equals_default_path():
    """The table-based kernels on the DEFAULT geometry (forced by an image size the register-resident path does not take: 42 px is
    no multiple of 12) against the oracle, and on a 48-px image against the register-resident path."""
    from oracle import bb
    from srganst.loss import BestBuddyLoss, _BestBuddyGeneralFn
    gen = torch.Generator().manual_seed(31)
    gt = torch.rand(2, 3, 48, 48, generator=gen)
    x = (gt + 0.1 * torch.randn(2, 3, 48, 48, generator=gen)).clamp(0, 1)
    mod = BestBuddyLoss()
    xa = x.cuda().requires_grad_(True)
    la = mod(xa, gt.cuda())
    la.backward()
    xb = x.cuda().requires_grad_(True)
    lb, indb = _BestBuddyGeneralFn.apply(xb, gt.cuda(), 1.0, 1.0, False, 3, 0, 3, 0, {})
    lb.backward()
    same = (indb == mod.last_index).float().mean().item()
    assert same > 0.99 and abs(la.item() - lb.item()) < 1e-4 * abs(la.item())
    if same == 1.0:
        assert rel_err(xb.grad, xa.grad) < 1e-6
    gt2 = torch.rand(1, 3, 42, 42, generator=gen)
    x2 = torch.rand(1, 3, 42, 42, generator=gen).requires_grad_(True)
    lo, io, score = bb.best_buddy_loss(x2, gt2)
    top2 = torch.topk(score, 2, dim=2, largest=False).values
    clear = ((top2[..., 1] - top2[..., 0]) > 1e-4).numpy()
    m2 = BestBuddyLoss()
    l2 = m2(x2.detach().cuda(), gt2.cuda())
    assert np.array_equal(m2.last_index.cpu().numpy()[clear], io.numpy()[clear]) and abs(l2.item() - lo.item()) < 1e-3 * abs(lo.item())


# ---- odd, non-square images (F.interpolate(scale_factor) maps coordinates with 1 / factor) and a 4 x 4 image with fewer candidates
# than the matcher's 8 candidate splits (tests/golden/bestbuddy_odd.npz, make_golden_bb_geom.py odd, from the reference itself)
GO = os.path.join(os.path.dirname(__file__), "golden", "bestbuddy_odd.npz")
ODD_CASES = {"h45w42": (3, 0, 3, "l2", "l1"), "h4w4": (3, 1, 3, "l2", "l2")}


@pytest.mark.parametrize("name", list(ODD_CASES))
def test_oracle_odd_size_matches_reference_golden(name):
    from oracle import bb
    k, pad, stride, dn, crit = ODD_CASES[name]
    g = np.load(GO)
    x = torch.from_numpy(g[f"{name}/x"]).requires_grad_(True)
    gt = torch.from_numpy(g[f"{name}/gt"])
    loss, ind, score = bb.best_buddy_loss(x, gt, ksize=k, pad=pad, stride=stride, dist_norm=dn, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    assert score.shape[2] == int(g[f"{name}/ncand"])
    assert torch.equal(loss.detach(), torch.from_numpy(g[f"{name}/loss"]))
    assert torch.equal(gx, torch.from_numpy(g[f"{name}/grad"]))
    assert np.array_equal(ind.numpy(), g[f"{name}/ind"])
    _, gt2, gt4 = bb.candidates(gt, k, pad, stride)
    assert torch.equal(gt2, torch.from_numpy(g[f"{name}/gt2"])) and torch.equal(gt4, torch.from_numpy(g[f"{name}/gt4"]))


def test_odd_size_fixture_covers_the_edges():
    g = np.load(GO)
    assert g["h45w42/x"].shape == (2, 3, 45, 42) and int(g["h45w42/ncand"]) == 210 + 49 + 9       # 15x14, 7x7 (22x21), 3x3 (11x10)
    assert not np.array_equal(g["h45w42/x"][0], g["h45w42/x"][1])
    assert int(g["h4w4/ncand"]) == 6 < 8                                                       # fewer candidates than the 8 splits


@pytest.mark.parametrize("fn", ["best_buddy_loss", "gram_loss", "patchwise_st_loss"])
@pytest.mark.parametrize("crit", ["l1", "l2"])
def test_oracle_fixed_selection(fn, crit):
    """ind= evaluates the loss at given buddies: at torch.min's own picks it is the unfixed loss bit for bit; at other picks it is
    the criterion against exactly those candidate rows."""
    from oracle import bb
    g = np.load(G["lf48"])
    x = torch.from_numpy(g["lf48/x"]).requires_grad_(True)
    gt = torch.from_numpy(g["lf48/gt"])
    f = getattr(bb, fn)
    loss, ind, score = f(x, gt, criterion=crit)
    (gx,) = torch.autograd.grad(loss, x)
    loss2, ind2, score2 = f(x, gt, criterion=crit, ind=ind.to(torch.int32))
    (gx2,) = torch.autograd.grad(loss2, x)
    assert torch.equal(loss, loss2) and torch.equal(gx, gx2) and torch.equal(ind, ind2) and torch.equal(score, score2)
    other = (ind + 1) % score.shape[2]
    loss3, ind3, _ = f(x, gt, criterion=crit, ind=other)
    assert torch.equal(ind3, other) and loss3.item() != loss.item()
