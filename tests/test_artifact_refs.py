"""CPU: the plain-torch restatement of ArtifactLoss (tests/artifact_refs.py) - held to a version with Python loops on a tiny case
and to autograd, its fp32 evaluation to its fp64 one, and its shared cases to the two conditions that keep the mask from hiding:
the masked share of every case lies in [0.25, 0.75], and no pixel sits closer than 1e-6 to the mask's boundary r = r_e."""
import pytest
import torch

import artifact_refs as refs


@pytest.mark.parametrize("with_ref", [True, False])
def test_restatement_equals_the_loop_version(with_ref):
    """4 x 4 at k = 7: every tap outside the centre column and row is a reflection."""
    sr, gt, ref = refs.images(*refs.CASES["tiny"][:4])
    ref = ref if with_ref else None
    want, wmap = refs.loop_loss(sr, gt, ref, 7)
    got = refs.artifact_loss(sr.double(), gt.double(), None if ref is None else ref.double(), 7)
    assert abs(got.item() - want) <= 1e-12 * abs(want) and want > 0
    w = refs.weight_map(sr.double(), gt.double(), None if ref is None else ref.double(), 7)
    want_w = torch.tensor(wmap, dtype=torch.float64).unsqueeze(1)
    assert torch.equal(w == 0, want_w == 0)                             # the same mask
    assert float((w - want_w).abs().max()) <= 1e-12 * float(want_w.abs().max())


def test_reflection_is_the_contracts():
    """Index -i reads i and H-1+i reads H-1-i: the window at a corner holds the mirrored block."""
    r = torch.arange(30, dtype=torch.float64).reshape(1, 1, 5, 6)
    v = refs.local_variance(r, 5)
    rows, cols = [2, 1, 0, 1, 2], [2, 1, 0, 1, 2]
    assert abs(v[0, 0, 0, 0].item() - r[0, 0][rows][:, cols].reshape(-1).var(unbiased=True).item()) < 1e-12
    rows, cols = [2, 3, 4, 3, 2], [3, 4, 5, 4, 3]
    assert abs(v[0, 0, 4, 5].item() - r[0, 0][rows][:, cols].reshape(-1).var(unbiased=True).item()) < 1e-12


@pytest.mark.parametrize("name", list(refs.CASES))
@pytest.mark.parametrize("with_ref", [True, False])
def test_autograd_gives_the_contracts_gradient(name, with_ref):
    """The map is a constant of the gradient: autograd through the restatement gives w sign(sr - gt) / (3 B H W), and nothing more."""
    sr, gt, ref, *_, g64 = refs.case(name, with_ref)
    k = refs.CASES[name][4]
    want = refs.analytic_grad(sr.double(), gt.double(), None if ref is None else ref.double(), k)
    assert want.shape == g64.shape and float((g64 - want).abs().max()) <= 1e-14 * float(want.abs().max())
    if with_ref:
        m = refs.mask(sr.double(), gt.double(), ref.double()).expand_as(g64)
        assert not bool(g64[m].any()) and bool((g64[~m] != 0).all())


@pytest.mark.parametrize("name", list(refs.CASES))
def test_cases_cannot_hide_the_mask(name):
    share, margin = refs.mask_facts(name)
    print(f"[{name}] masked share {share:.4f}, min |r - r_e| {margin:.3e}")
    assert 0.25 <= share <= 0.75
    assert margin >= 1e-6


@pytest.mark.parametrize("name", list(refs.CASES))
def test_fp32_agrees_with_fp64(name):
    for with_ref in (True, False):
        _, _, _, l32, g32, l64, g64 = refs.case(name, with_ref)
        assert abs(l32 - l64).item() <= 1e-5 * abs(l64).item()
        assert float((g32 - g64).abs().max()) <= 1e-5 * float(g64.abs().max())


def test_exact_consequences():
    sr, gt, ref = refs.images(7, 2, 12, 9)
    assert refs.artifact_loss(gt.clone(), gt).item() == 0.0             # sr == gt: r = 0, both variances 0
    _, g = refs.loss_and_grad(gt.clone(), gt, None, 7)
    assert not bool(g.any())
    for dtype in (torch.float32, torch.float64):                        # ref is sr: the strict comparison masks nothing
        a, b = sr.to(dtype), gt.to(dtype)
        assert torch.equal(refs.artifact_loss(a, b, a), refs.artifact_loss(a, b))
    assert refs.artifact_loss(sr, gt, ref).item() < refs.artifact_loss(sr, gt).item()
