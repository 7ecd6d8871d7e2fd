"""CPU: the restatement of the back-projection criterion (tests/bp_refs.py) held to the project's own resampler (bicubic.Bicubic), its
dense adjoint checked, and the two margins asserted that keep the GPU parity tests honest.

Where fp32 and fp64 disagree on the sign of a D, an L1 gradient differs by a whole tap footprint, and no tolerance should absorb
that: every case used with "l1" has min |D| >= 1e-5 in the fp64 restatement (about 50 x the largest fp32 error of D).  "mse" needs
no such condition."""
import pytest
import torch

import bp_refs as refs


def _bicubic_unrounded(gt, s):
    """Bicubic("cpu").forward before its rounding: the gather-multiply-sum over the tap tables, in fp32."""
    from srganst.bicubic import Bicubic
    w0, i0, w1, i1 = Bicubic("cpu").tables(gt.shape[2], gt.shape[3], 1.0 / s, "cpu")
    out = torch.sum(gt[:, :, i0, :] * w0[None, None, :, :, None], dim=3)
    A = out.permute(0, 1, 3, 2)
    return torch.sum(A[:, :, i1, :] * w1[None, None, :, :, None], dim=3).permute(0, 1, 3, 2)


@pytest.mark.parametrize("name", list(refs.CASES))
def test_restatement_is_the_projects_resampler(name):
    from srganst.bicubic import Bicubic
    B, H, W, s, _ = refs.CASES[name]
    sr, gt, T_round, T_plain, _ = refs.inputs(name)
    assert tuple(T_round.shape) == (B, 3, int(H * (1.0 / s)), int(W * (1.0 / s)))
    assert bool((gt == torch.round(gt * 255) / 255).all()) and 0 <= float(gt.min()) and float(gt.max()) <= 1
    for x in (gt, sr):
        e = (refs.down(x, s) - _bicubic_unrounded(x, s)).abs().max().item()
        assert e <= 2e-6, e                                   # ~1e-6: two fp32 summation orders of values in [0, 1]
    # no value of 255 down(gt) sits at a rounding tie, so the rounded restatement IS the LR image the dataset makes
    assert refs.tie_distance(name) >= refs.TIE_MARGIN
    assert torch.equal(T_round, Bicubic("cpu")(gt, 1.0 / s))
    assert float((T_round - T_plain).abs().max()) <= 0.5 / 255 + 1e-6 and not torch.equal(T_round, T_plain)


@pytest.mark.parametrize("name", list(refs.CASES))
def test_dense_adjoint(name):
    _, H, W, s, seed = refs.CASES[name]
    My, Mx = refs.matrices(H, W, s)
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float64)
    v = torch.randn(2, 3, My.shape[0], Mx.shape[0], generator=gen, dtype=torch.float64)
    lhs, rhs = (refs.down(u, s) * v).sum(), (u * (My.t() @ v @ Mx)).sum()
    assert abs(lhs - rhs).item() <= 1e-12 * max(1.0, abs(lhs).item())
    assert torch.allclose(My.sum(dim=1), torch.ones(My.shape[0], dtype=torch.float64), atol=1e-6)      # normalised weights
    # autograd's gradient of the restatement is that adjoint
    x = u.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((refs.down(x, s) * v).sum(), x)
    assert (g - My.t() @ v @ Mx).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", refs.L1_CASES)
def test_l1_cases_keep_their_margin(name):
    m = refs.min_abs_d(name)
    assert m >= refs.L1_MARGIN, f"{name}: min |D| = {m:.3e} in fp64"
    sr, _, T, _, s = refs.inputs(name)
    e32 = (refs.down(sr, s).double() - refs.down(sr.double(), s)).abs().max().item()
    assert e32 <= refs.L1_MARGIN / 20, e32                    # the fp32 error of D the margin is sized for
    # so fp32 and fp64 agree on every sign, and the two L1 gradients differ by rounding only
    *_, g32, _, g64 = refs.case(name, "l1")
    assert (g32 - g64).abs().max().item() <= 1e-5 * g64.abs().max().item()


def test_cases_are_the_table():
    assert set(refs.L1_CASES) <= set(refs.CASES) and len(refs.CASES) == 8
    lr = {n: (int(H * (1.0 / s)), int(W * (1.0 / s))) for n, (_, H, W, s, _) in refs.CASES.items()}
    assert lr == {"one output": (1, 1), "ragged": (3, 5), "narrow": (2, 25), "wide": (2, 275), "medium": (12, 10), "x2": (15, 13),
                  "x8": (8, 5), "crop": (24, 24)}
