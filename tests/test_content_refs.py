"""The CPU references of the feature criteria that tests/test_content_losses_fp64_gpu.py holds the HIP path to (tests/content_refs.py
over oracle/vgg.py and oracle/model.py).  Two things:
  - what was added to the oracle is plain torch: the L1 criterion of oracle.vgg.content_loss, nested tap sets, the seeded states;
  - the condition the GPU bounds rest on: at every rung of both ladders the oracle evaluated in fp32 is within 1e-4 of the oracle
    evaluated in fp64, for the loss and for d loss / d sr.  conftest.truth_bound is max(1e-3, 3 x that distance), so the condition
    pins every gradient bound of the GPU file to the 1e-3 floor and every loss bound to 1e-4: the rule cannot widen itself.
    For the L1 criterion the gradient distance is content_refs.Ref.grad_err (the tap elements no fp32 evaluation can decide are
    fitted, everything else is held norm-wise); the plain norm-wise figure is printed next to it."""
import pytest
import torch
import torch.nn.functional as F

import content_refs as cr
from conftest import rel_err


def test_vgg_l1_criterion_is_l1_loss_of_the_features():
    from oracle import vgg as ovgg
    sd = cr.vgg_state()
    x, gt = cr.images(b=1, h=16, w=24)
    taps = {3: 0.3, 8: 0.7}
    fx, fg = ovgg.vgg_features(sd, x, (3, 8)), ovgg.vgg_features(sd, gt, (3, 8))
    want = sum(w * F.l1_loss(fx[k], fg[k]) for k, w in taps.items())
    assert torch.equal(ovgg.content_loss(sd, x, gt, cr.layers(taps), "l1"), want)
    want = sum(w * F.mse_loss(fx[k], fg[k]) for k, w in taps.items())
    assert torch.equal(ovgg.content_loss(sd, x, gt, cr.layers(taps), "l2"), want)
    assert torch.equal(ovgg.content_loss(sd, x, gt, cr.layers(taps)), want)
    with pytest.raises(NotImplementedError):
        ovgg.content_loss(sd, x, gt, cr.layers(taps), "huber")


def test_vgg_nested_tap_sets_give_identical_features():
    """A tap's features do not depend on which other taps are asked for (the ladder's rungs are prefixes of one stack)."""
    from oracle import vgg as ovgg
    sd = cr.vgg_state()
    x, _ = cr.images(b=1, h=16, w=32)
    every = ovgg.vgg_features(sd, x, cr.VGG_RUNGS)
    assert sorted(every) == list(cr.VGG_RUNGS)
    for taps in ((1,), (1, 3), (8, 22, 24), (17, 26, 35), (35,)):
        got = ovgg.vgg_features(sd, x, taps)
        assert sorted(got) == list(taps)
        for k in taps:
            assert torch.equal(got[k], every[k]), (taps, k)
    assert every[35].shape == (1, 512, 1, 2) and bool((every[35] >= 0).all())


def test_seeded_states_are_what_they_claim():
    from oracle import model as om
    from oracle import vgg as ovgg
    plain, biased = ovgg.init_vgg_state(cr.VGG_SEED), cr.vgg_state()
    for k in plain:
        if k.endswith(".weight"):
            assert torch.equal(plain[k], biased[k]), k
        else:
            assert not bool(plain[k].any()) and 0.05 < float(biased[k].std()) < 0.2, k
    sd = cr.disc_state()
    assert all(k.startswith("features.") for k in sd)
    for ci, bi, _, om_, _ in om.D_PLAN:
        assert sd[f"features.{ci}.weight"].shape[0] == 64 * om_
        if bi is None:
            assert bool(sd[f"features.{ci}.bias"].any())
            continue
        rv, gamma = sd[f"features.{bi}.running_var"], sd[f"features.{bi}.weight"]
        assert float(rv.min()) >= 0.5 and float(rv.max()) <= 1.5 and float(gamma.min()) >= 0.5 and float(gamma.max()) <= 1.5
        assert float(sd[f"features.{bi}.running_mean"].abs().max()) > 0.1 and float(sd[f"features.{bi}.bias"].abs().max()) > 0.05
    torch.manual_seed(123)
    a = torch.rand(1)
    torch.manual_seed(123)
    cr._STATES.pop(("disc", 99, 64), None)
    cr.disc_state(99)                                # seeds inside a forked RNG: the caller's stream is left alone
    assert torch.equal(torch.rand(1), a)


def _condition(label, ref):
    e_loss, e_grad = ref.loss_err(ref.loss32), ref.grad_err(ref.grad32)
    print(f"[{label}] fp32 oracle vs fp64 oracle: loss {e_loss:.2e}, d/d sr {e_grad:.2e} (plain {rel_err(ref.grad32, ref.grad64):.2e}, "
          f"{ref.undecided} undecidable L1 signs)")
    assert float(ref.loss64) > 0 and float(ref.grad64.norm()) > 0
    assert e_loss <= cr.FP32_ORACLE_CONDITION and e_grad <= cr.FP32_ORACLE_CONDITION, (label, e_loss, e_grad)
    assert ref.loss_bound() == 1e-4 and ref.grad_bound() == 1e-3            # what the GPU file will hold the HIP path to


@pytest.mark.parametrize("label,taps,crit", cr.vgg_cases(), ids=[c[0] for c in cr.vgg_cases()])
def test_vgg_fp32_oracle_within_1e4_of_fp64(label, taps, crit):
    _condition("vgg " + label, cr.vgg_ref(taps, crit))


@pytest.mark.parametrize("label,taps,crit", cr.disc_cases(), ids=[c[0] for c in cr.disc_cases()])
def test_disc_fp32_oracle_within_1e4_of_fp64(label, taps, crit):
    _condition("disc " + label, cr.disc_ref(taps, crit))


def test_vgg_96px_point_fp32_oracle_within_1e4_of_fp64():
    """The existing 96-px point of tests/test_vgg_gpu.py (B = 2, image seed 8, default taps, state seed 7) with non-zero biases."""
    _condition("vgg 96 px default taps", cr.vgg_ref(cr.VGG_SETS["default"], image=cr.IMAGE_96))


@pytest.mark.parametrize("kind", ["vgg", "disc"])
def test_l1_gradient_distance_fits_undecidable_elements_only(kind):
    """Ref.grad_err: an undecidable element may take any value a sign / mask could give it and nothing else; everything decidable
    is measured norm-wise as usual."""
    refs = [cr.vgg_ref({k: 1.0}, "l1") for k in cr.VGG_L1_RUNGS] if kind == "vgg" else [cr.disc_ref({k: 1.0}, "l1") for k in cr.DISC_RUNGS]
    ref = next(r for r in refs if r.undecided >= 2)
    g, k = ref.grad64, ref.undecided
    gen = torch.Generator().manual_seed(0)
    assert ref.grad_err(g) == 0.0
    c = ref.allowed[torch.randint(len(ref.allowed), (k,), generator=gen)]
    other = ref.decided + (c @ ref.basis).view_as(g)
    assert ref.grad_err(other) < 1e-12 and ref.grad_err(ref.decided) < 1e-12
    c[0] = 3.0                                                                  # ... but never more than weight / N
    far = ref.decided + (c @ ref.basis).view_as(g)
    want = float((2.0 * ref.basis[0]).norm() / g.norm())
    assert abs(ref.grad_err(far) - want) < 1e-3 * want and want > 1e-4
    assert abs(ref.grad_err(g * 1.01) - 0.01) < 1e-3
    noise = torch.randn(g.shape, generator=gen, dtype=torch.float64)
    assert abs(ref.grad_err(other + 0.01 * g.norm() / noise.norm() * noise) - 0.01) < 1e-3
