"""The two feature criteria, ContentLossVGG (srganst/vgg_loss.py) and ContentLossDiscriminator (srganst/disc_loss.py), on the GPU
against their oracles evaluated in fp64 (tests/content_refs.py; the references themselves: tests/test_content_refs.py), tap by tap.

Every numeric case: B = 3, 32 x 48 px (not square, the 2B batch is 6, 2 x 3 is left after four halvings), SR = (gt + 0.1 * randn)
clamped, full width, VGG with non-zero biases loaded from a weight file, the discriminator with a non-trivial eval-mode BatchNorm,
an upstream gradient of -0.37 as a device scalar.  Bounds (fixed by the rule, not by what is measured):
  loss      within max(1e-4, 3 x the fp32 oracle's distance from the fp64 oracle)
  d / d sr  conftest's fp64-truth rule, max(1e-3, 3 x the fp32 oracle's distance); for the L1 criterion the distance leaves the tap
            elements that no fp32 evaluation can decide free to take any value a sign / mask can give them (content_refs.Ref).
tests/test_content_refs.py holds the fp32 oracle within 1e-4 at every rung, so these are 1e-4 and 1e-3 throughout.
`-s` prints the ladders; `python tests/test_content_losses_fp64_gpu.py` prints the VGG ladder at 96 px with and without biases
("Feature criteria against fp64")."""
import pytest
import torch

import content_refs as cr
from graph_refs import graph_vs_eager

pytestmark = pytest.mark.gpu

UPSTREAM = -0.37
REPORT = {"vgg": [], "disc": []}


@pytest.fixture(scope="module", autouse=True)
def _print_reports():
    yield
    for kind, rows in REPORT.items():
        if rows:
            print(f"\n{kind} ladder, B = {cr.B}, {cr.H} x {cr.W}: case, |hip - fp64| loss / grad, |fp32 oracle - fp64| loss / grad, undecidable")
            for r in rows:
                print("  %-18s hip %.2e / %.2e   fp32 oracle %.2e / %.2e   %d" % r)


def _vgg_file(tmp_path, biased=True, seed=cr.VGG_SEED):
    path = tmp_path / "vgg19.pth"
    torch.save(dict(cr.vgg_state(seed, biased)), path)
    return str(path)


def _vgg_module(weights, taps, crit="mse"):
    from srganst.config import Config
    from srganst.loss import ContentLossVGG
    cfg = Config()
    cfg.MODEL.G_LOSS.VGG19_LAYERS = cr.layers(taps)
    return ContentLossVGG(cfg, criterion=crit, weights=weights, seed=1)


def _disc_module(taps, crit="mse", state=True):
    from srganst.config import Config
    from srganst.loss import ContentLossDiscriminator
    cfg = Config()
    cfg.MODEL.G_LOSS.DISC_FEATURES_LOSS_LAYERS = cr.layers(taps)
    mod = ContentLossDiscriminator(cfg, criterion=crit)
    if state:
        res = mod.D.load_state_dict({k: v for k, v in cr.disc_state().items()}, strict=False)
        assert not res.unexpected_keys and all(k.startswith("classifier.") for k in res.missing_keys)
    return mod


def _run(mod, x, gt, upstream=UPSTREAM):
    """-> (loss, d loss / d sr) of the HIP module, the gradient taken through a device scalar `upstream` and divided out again."""
    xg = x.cuda().requires_grad_(True)
    loss = mod(xg, gt.cuda())
    assert loss.shape == () and loss.dtype == torch.float32
    (loss * upstream).backward()
    return loss.detach().cpu(), xg.grad.cpu().double() / upstream


def _hold(label, kind, loss, grad, ref):
    e_loss, e_grad = ref.loss_err(loss), ref.grad_err(grad)
    row = (label, e_loss, e_grad, ref.loss_err(ref.loss32), ref.grad_err(ref.grad32), ref.undecided)
    if kind:
        REPORT[kind].append(row)
    print("[%s] hip %.2e / %.2e   fp32 oracle %.2e / %.2e   undecidable %d" % row)
    assert torch.isfinite(grad).all()
    assert e_loss <= ref.loss_bound(), f"{label} loss: |hip - fp64| = {e_loss:.3e} > {ref.loss_bound():.3e}"
    assert e_grad <= ref.grad_bound(), f"{label} d/d sr: |hip - fp64| = {e_grad:.3e} > {ref.grad_bound():.3e}"


# ---- 1 + 2: VGG depth ladder and tap sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,taps,crit", cr.vgg_cases(), ids=[c[0] for c in cr.vgg_cases()])
def test_vgg_taps_vs_fp64(label, taps, crit, tmp_path):
    """One module per ReLU of features[0..35] (MSE; L1 at 1, 8, 22, 35), then tap sets the backward never saw: both taps of the first
    block (the three-channel conv), mid-stack taps (the criterion gradient accumulates onto bwd_apply's output), the default
    (pool-adjacent and last), and a mid-stack tap with a pool-adjacent one in the same block."""
    mod = _vgg_module(_vgg_file(tmp_path), taps, crit)
    x, gt = cr.images()
    _hold(label, "vgg", *_run(mod, x, gt), cr.vgg_ref(taps, crit))


# ---- 3: discriminator-feature ladder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,taps,crit", cr.disc_cases(), ids=[c[0] for c in cr.disc_cases()])
def test_disc_taps_vs_fp64(label, taps, crit):
    """Every LeakyReLU of the discriminator's feature stack, MSE and L1: features.1 (no BatchNorm: null scale / shift in
    sst_feat_loss_*), the stride-2 data gradients of layers 2, 8, 14 and 20, and one set over three depths."""
    mod = _disc_module(taps, crit)
    x, gt = cr.images()
    _hold(label, "disc", *_run(mod, x, gt), cr.disc_ref(taps, crit))


# ---- 4: the 96-px point of tests/test_vgg_gpu.py, with biases --------------------------------------------------------------------
def test_vgg_96px_default_taps_with_biases_vs_fp64(tmp_path):
    """B = 2, 96 px, image seed 8, state seed 7, default taps - the input tests/test_vgg_gpu.py accepts at 4e-3 with zero biases -
    with non-zero biases: the fp32 oracle is within 1e-5 of the fp64 one there, so the bounds are 1e-4 / 1e-3."""
    taps = cr.VGG_SETS["default"]
    mod = _vgg_module(_vgg_file(tmp_path), taps)
    x, gt = cr.images(*cr.IMAGE_96)
    _hold("96px default", None, *_run(mod, x, gt), cr.vgg_ref(taps, image=cr.IMAGE_96))


def ladder_96px():
    """Not a test (no bound): the VGG ladder at the 96-px point, with and without biases, HIP error next to the fp32 oracle's - norm-wise
    against the fp64 oracle, and again with the ReLU masks no fp32 evaluation can decide fitted (content_refs.vgg_mask_ref)."""
    import tempfile
    from pathlib import Path
    from conftest import rel_err
    for biased in (True, False):
        print(f"VGG ladder at B = 2, 96 x 96 (image seed 8, state seed 7), {'biases 0.1 * randn' if biased else 'zero biases'}: tap, undecidable "
              "masks k; |hip - fp64| loss, grad, grad with the k masks fitted; the same for the fp32 oracle")
        with tempfile.TemporaryDirectory() as tmp:
            weights = _vgg_file(Path(tmp), biased)
            for taps in [{k: 1.0} for k in cr.VGG_RUNGS] + [cr.VGG_SETS["default"]]:
                ref = cr.vgg_mask_ref(taps, biased=biased, image=cr.IMAGE_96)
                loss, grad = _run(_vgg_module(weights, taps), *cr.images(*cr.IMAGE_96))
                print("  %-9s k %2d   hip %.2e  %.2e  %.2e   fp32 oracle %.2e  %.2e  %.2e" % (
                    "+".join(map(str, taps)), ref.undecided, ref.loss_err(loss), rel_err(grad, ref.grad64), ref.grad_err(grad),
                    ref.loss_err(ref.loss32), rel_err(ref.grad32, ref.grad64), ref.grad_err(ref.grad32)), flush=True)


# ---- 5: host-side behaviour ----------------------------------------------------------------------------------------------------
def _modules(kind, tmp_path):
    """-> a factory of identical modules with taps over several depths."""
    if kind == "vgg":
        weights = _vgg_file(tmp_path)
        return lambda: _vgg_module(weights, {8: 0.5, 17: 0.25, 35: 0.25})
    return lambda: _disc_module({1: 0.2, 13: 0.3, 22: 0.5})


def _loss_grad(mod, x, gt):
    xg = x.cuda().requires_grad_(True)
    loss = mod(xg, gt.cuda())
    loss.backward()
    return loss.detach().clone(), xg.grad.clone()


@pytest.mark.parametrize("kind", ["vgg", "disc"])
def test_workspaces_rekey_between_batch_sizes(kind, tmp_path):
    """B = 3, then B = 1, then B = 3 again on one module (the per-tap partials / counters of _ws are keyed by size): every call equals
    the same call on a fresh module bit for bit."""
    make = _modules(kind, tmp_path)
    x, gt = cr.images()
    mod = make()
    for sl in (slice(0, 3), slice(1, 2), slice(0, 3)):
        got, want = _loss_grad(mod, x[sl], gt[sl]), _loss_grad(make(), x[sl], gt[sl])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), sl
        assert bool(got[1].any())


@pytest.mark.parametrize("kind", ["vgg", "disc"])
def test_no_grad_paths_save_nothing_and_gt_gets_no_gradient(kind, tmp_path):
    mod = _modules(kind, tmp_path)()
    x, gt = cr.images()
    want, gwant = _loss_grad(mod, x, gt)
    with torch.no_grad():
        l1 = mod(x.cuda().requires_grad_(True), gt.cuda())
    l2 = mod(x.cuda(), gt.cuda())                                   # sr does not ask for a gradient
    for l in (l1, l2):
        assert torch.equal(l, want) and l.grad_fn is None and not l.requires_grad
    xg, gg = x.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
    l3 = mod(xg, gg)
    l3.backward()
    assert torch.equal(l3.detach(), want) and gg.grad is None and torch.equal(xg.grad, gwant)
    gg = gt.cuda().requires_grad_(True)                             # only gt asks: the forward keeps nothing, backward gives None
    l4 = mod(x.cuda(), gg)
    l4.backward()
    assert torch.equal(l4.detach(), want) and gg.grad is None
    assert l4.grad_fn is not None and not hasattr(l4.grad_fn, "saved") and not hasattr(l4.grad_fn, "module")


def test_vgg_refuses_odd_pool_input_and_recovers(tmp_path):
    """40 x 48 with a tap at 35: the fourth MaxPool2d(2) would see 5 rows - HipPathError, and the next valid call on the same module
    is what it was before."""
    from srganst._abi import HipPathError
    mod = _vgg_module(_vgg_file(tmp_path), {35: 1.0})
    x, gt = cr.images()
    want = _loss_grad(mod, x, gt)
    xo, go = cr.images(b=2, h=40, w=48)
    with pytest.raises(HipPathError):
        mod(xo.cuda().requires_grad_(True), go.cuda())
    torch.cuda.synchronize()
    got = _loss_grad(mod, x, gt)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_taps_that_are_not_activations_are_refused(tmp_path):
    weights = _vgg_file(tmp_path)
    for bad in (2, 4, 0, 36):                                        # a conv, a pool, the first conv, past features[35]
        with pytest.raises(NotImplementedError):
            _vgg_module(weights, {bad: 1.0})
    with pytest.raises(NotImplementedError):
        _vgg_module(weights, {17: 0.5, 2: 0.5})
    for bad in (0, 2, 3, 5, 21, 23):                                 # convs, BatchNorms, past the last LeakyReLU
        with pytest.raises(NotImplementedError):
            _disc_module({bad: 1.0}, state=False)
    with pytest.raises(NotImplementedError):
        _disc_module({4: 0.5, 9: 0.5}, state=False)


# ---- 6: captured step equals eager step ----------------------------------------------------------------------------------------
def _reported_equals_standalone(names):
    def check(eng, cfg, gt):
        """_criterion_total reports weight * criterion(sr, gt), detached."""
        for name in names:
            crit, w = cfg.MODEL.G_LOSS.CRITERIONS[name], cfg.MODEL.G_LOSS.CRITERION_WEIGHTS[name]
            want = (crit(eng.sr, gt) * w).detach()
            got = eng.loss_values[name]
            assert float(got) != 0.0 and torch.equal(got, want), (name, float(got), float(want))
    return check


@pytest.mark.parametrize("schedule", ["shared", "batched"])
@pytest.mark.parametrize("terms", ["ContentVGG", "ContentDiscriminator", "ContentVGG+ContentDiscriminator"])
def test_train_engine_graph_equals_eager_with_feature_criteria(terms, schedule):
    """Adversarial + Pixel + ST + ContentVGG (seeded-random weights; weight 1) and / or ContentDiscriminator (weight 2000) through
    TrainEngine: the captured iteration equals the eager one bit for bit over 5 iterations under both discriminator schedules, and
    after the first eager step each reported value is the criterion applied stand-alone to eng.sr and gt, times its weight."""
    from srganst.loss import ContentLossDiscriminator, ContentLossVGG
    names = terms.split("+")
    make = {"ContentVGG": lambda cfg: ContentLossVGG(cfg, allow_random=True), "ContentDiscriminator": ContentLossDiscriminator}
    graph_vs_eager(lambda cfg: [(n, make[n](cfg)) for n in names], schedule == "shared", _reported_equals_standalone(names))


if __name__ == "__main__":
    ladder_96px()
