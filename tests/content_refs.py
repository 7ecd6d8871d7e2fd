"""Shared CPU references of the two feature criteria (ContentLossVGG, ContentLossDiscriminator) for tests/test_content_refs.py
(not gpu: the references against plain torch, and the fp32-oracle condition the GPU bounds rest on) and
tests/test_content_losses_fp64_gpu.py (the HIP path against them).  Everything is oracle/ code evaluated in fp32 and in fp64;
each case is computed once per process and handed out read-only."""
from collections import OrderedDict

import torch

from conftest import TRUTH_FACTOR, TRUTH_FLOOR

# ---- the cases (issue: every rung at B = 3, 32 x 48: not square, the 2B batch is 6, 2 x 3 is left after four halvings) -----------
B, H, W = 3, 32, 48
VGG_SEED, DISC_SEED, IMAGE_SEED = 7, 5, 3
IMAGE_96 = (8, 2, 96, 96)          # (seed, B, H, W) of the existing 96-px point of tests/test_vgg_gpu.py
VGG_RUNGS = (1, 3, 6, 8, 11, 13, 15, 17, 20, 22, 24, 26, 29, 31, 33, 35)          # every ReLU of features[0..35]
VGG_L1_RUNGS = (1, 8, 22, 35)
VGG_SETS = OrderedDict([
    ("first-block", {1: 0.3, 3: 0.7}),                      # taps on the three-channel conv and its neighbour
    ("mid-stack", {8: 0.5, 22: 0.25, 24: 0.25}),            # taps whose gradient accumulates onto bwd_apply's output
    ("default", {17: 1 / 8, 26: 1 / 4, 35: 1 / 2}),
    ("pool-and-mid", {15: 0.5, 17: 0.5}),                   # a mid-stack tap and a pool-adjacent one in the same block
])
DISC_RUNGS = (1, 4, 7, 10, 13, 16, 19, 22)
DISC_SET = {1: 0.2, 13: 0.3, 22: 0.5}
FP32_ORACLE_CONDITION = 1e-4      # fp32 oracle within this of the fp64 oracle at every rung => the fp64-truth bound is its 1e-3 floor


def layers(taps):
    return {f"features.{k}": float(w) for k, w in taps.items()}


def vgg_cases():
    """[(id, {tap: weight}, criterion)] of the VGG ladder and tap sets."""
    out = [(f"relu{k}-mse", {k: 1.0}, "mse") for k in VGG_RUNGS]
    out += [(f"relu{k}-l1", {k: 1.0}, "l1") for k in VGG_L1_RUNGS]
    out += [(f"{name}-mse", taps, "mse") for name, taps in VGG_SETS.items()]
    return out


def disc_cases():
    out = [(f"lrelu{k}-{c}", {k: 1.0}, c) for c in ("mse", "l1") for k in DISC_RUNGS]
    out += [(f"mixed-{c}", DISC_SET, c) for c in ("mse", "l1")]
    return out


def images(seed=IMAGE_SEED, b=B, h=H, w=W):
    """-> (sr, gt): GT uniform in [0, 1], SR = (gt + 0.1 * randn).clamp(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(b, 3, h, w, generator=g)
    return (gt + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1), gt


# ---- seeded states ------------------------------------------------------------------------------------------------------------
_STATES = {}


def vgg_state(seed=VGG_SEED, biased=True):
    from oracle import vgg as ovgg
    key = ("vgg", seed, biased)
    if key not in _STATES:
        _STATES[key] = (ovgg.init_vgg_state_biased if biased else ovgg.init_vgg_state)(seed)
    return _STATES[key]


def disc_state(seed=DISC_SEED, ch=64):
    """`features.*` of a seeded discriminator whose eval-mode BatchNorm is far from the identity a fresh one has (mean 0, var 1,
    gamma 1, beta 0): the draws of tests/golden/make_golden_dfeat.py per BatchNorm - running_mean 0.2 * randn, running_var
    rand + 0.5, gamma rand + 0.5, beta 0.1 * randn, in that order from one generator (seed + 1) - and a conv bias 0.1 * randn."""
    from oracle import model as om
    key = ("disc", seed, ch)
    if key in _STATES:
        return _STATES[key]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        full = om.init_discriminator_state(ch=ch, image_size=16)        # image_size: only sizes the classifier, which is dropped
    sd = OrderedDict((k, v) for k, v in full.items() if k.startswith("features."))
    g = torch.Generator().manual_seed(seed + 1)
    for ci, bi, _, _, _ in om.D_PLAN:
        if bi is None:
            sd[f"features.{ci}.bias"] = 0.1 * torch.randn(sd[f"features.{ci}.bias"].shape, generator=g)
            continue
        n = sd[f"features.{bi}.weight"].numel()
        sd[f"features.{bi}.running_mean"] = 0.2 * torch.randn(n, generator=g)
        sd[f"features.{bi}.running_var"] = torch.rand(n, generator=g) + 0.5
        sd[f"features.{bi}.weight"] = torch.rand(n, generator=g) + 0.5
        sd[f"features.{bi}.bias"] = 0.1 * torch.randn(n, generator=g)
    _STATES[key] = sd
    return sd


# ---- the oracle in fp32 and in fp64 ---------------------------------------------------------------------------------------------
# MSE: d loss / d sr is continuous in the features, and the fp32 oracle sits within 1e-5 of the fp64 one.
# L1: the gradient at a tap element is weight / N * sign(d) * act'(z_sr) with d = act(z_sr) - act(z_gt), and among the 10^4..10^5
# elements of a tap a few have a d (or a z_sr) smaller than the rounding of ANY fp32 evaluation (measured at lrelu22: median |d|
# 1e-4, smallest 1e-10, fp32 error on d 1e-8).  Each such element moves the norm-wise gradient error by ~ 1 / sqrt(N) ~ 1e-3..1e-2
# whichever way it falls - the fp32 oracle itself lands 1.3e-3..6.8e-3 from the fp64 one at 6 of the 13 L1 cases.  (Under MSE the
# same element weighs d itself, i.e. nothing.)  So for L1 the elements that fp32 cannot decide - |d| < delta or |z_sr| < delta (unless
# act(z_sr + delta) = 0: no gradient either way), delta = 3 x the fp32 oracle's largest error on z and d at that tap - are taken out
# of the fp64 gradient and kept as a basis V (weight / N * d z_sr[i] / d sr, one back-propagated unit vector each).  A gradient g
# is measured against
#     g64_decided + V c,   c_i in {sign * act'} = {-1, 0, +1} (ReLU) or {-1, -0.2, 0, +0.2, +1} (LeakyReLU 0.2)
# with c = the least-squares fit of g - g64_decided on V, rounded to the nearest allowed value: every decidable element is held to
# the full bound, and an undecidable one must still contribute exactly one of the values some sign / mask gives it.  With no
# undecidable element (and for MSE) this is the plain norm-wise error against the fp64 oracle.
MAX_UNDECIDED = 128       # of >= 9216 tap elements, against 13 824 gradient entries: the fit stays far over-determined.  More than
                          # that and the input would soften the L1 check: the reference refuses


class Ref:
    """loss32 / grad32 / loss64 / grad64: oracle results.  L1 only (see above): decided = g64_decided, basis [k, numel] or None,
    allowed = the values a coefficient may take."""

    def __init__(self, l32, g32, l64, g64, decided=None, basis=None, allowed=None):
        self.loss32, self.grad32, self.loss64, self.grad64 = l32, g32, l64, g64
        self.decided, self.basis, self.allowed = decided, basis, allowed

    @property
    def undecided(self):
        return 0 if self.basis is None else self.basis.shape[0]

    def grad_err(self, g):
        """Norm-wise error of g against the fp64 gradient, the undecidable L1 coefficients fitted and rounded."""
        g = torch.as_tensor(g).detach().to(torch.float64).cpu()
        ref = self.grad64
        plain = float((g - ref).norm() / ref.norm())
        if self.basis is None:
            return plain
        r = (g - self.decided).flatten()
        v = self.basis[self.basis.norm(dim=1) > 0].t()              # an element nothing downstream listens to has a zero row
        if v.shape[1] == 0:
            return plain
        c = torch.linalg.lstsq(v, r.unsqueeze(1), driver="gelsd").solution.squeeze(1)
        c = self.allowed[(c.unsqueeze(1) - self.allowed.unsqueeze(0)).abs().argmin(dim=1)]
        return min(plain, float((r - v @ c).norm() / ref.norm()))

    def loss_err(self, loss):
        return rel_loss_err(loss, self.loss64)

    def loss_bound(self):
        return max(1e-4, 3.0 * self.loss_err(self.loss32))

    def grad_bound(self):
        """conftest.truth_bound with grad_err as the distance."""
        return max(TRUTH_FLOOR, TRUTH_FACTOR * self.grad_err(self.grad32))


_REFS = {}


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _loss_and_grad(fn, x, gt, dtype):
    x = x.detach().to(dtype).requires_grad_(True)
    loss = fn(x, gt.to(dtype))
    (gx,) = torch.autograd.grad(loss, x)
    return loss.detach(), gx


def _l1_split(pre, act, sd, taps, x, gt, g64):
    """pre(sd, a) -> {tap: pre-activation z}, act: the tap's activation.  -> (gradient of the decidable part of
    sum_t w_t * mean |act(z_t(x)) - act(z_t(gt))| in fp64, basis of the undecidable elements or None)."""
    sd64, sd32 = _cast(sd, torch.float64), _cast(sd, torch.float32)
    x64 = x.detach().double().requires_grad_(True)
    zx, zg = pre(sd64, x64), pre(sd64, gt.double())
    with torch.no_grad():
        zx32, zg32 = pre(sd32, x.float()), pre(sd32, gt.float())
    decided, units, coef = 0.0, [], []
    for t, w in taps.items():
        a, b = zx[t].flatten(), zg[t].flatten()
        d = act(a) - act(b)
        av, dv = a.detach(), d.detach()
        a32, b32 = zx32[t].flatten(), zg32[t].flatten()
        err = lambda v32, v64: float((v32.double() - v64).abs().max())
        delta = 3.0 * max(err(a32, av), err(b32, b.detach()), err(act(a32) - act(b32), dv))
        dead = (act(av + delta) == 0)                               # act'(z_sr) = 0 in any fp32 evaluation: nothing to decide
        und = ~dead & ((dv.abs() < delta) | (av.abs() < delta))
        decided = decided + (w / d.numel()) * d[~und].abs().sum()
        idx = und.nonzero().flatten().tolist()
        units += [(w / d.numel()) * a[i] for i in idx]
        if idx:
            ai = av[idx].clone().requires_grad_(True)
            (slope,) = torch.autograd.grad(act(ai).sum(), ai)
            coef += (torch.sign(dv[idx]) * slope).tolist()          # what the fp64 oracle gives these elements
    assert len(units) <= MAX_UNDECIDED, f"{len(units)} tap elements undecidable in fp32: pick another input"
    (g_dec,) = torch.autograd.grad(decided, x64, retain_graph=bool(units))
    if not units:
        assert float((g_dec - g64).norm() / g64.norm()) < 1e-12
        return g_dec, None
    basis = torch.stack([torch.autograd.grad(u, x64, retain_graph=True)[0].flatten() for u in units])
    restated = g_dec + (torch.tensor(coef, dtype=torch.float64) @ basis).view_as(g_dec)
    assert float((restated - g64).norm() / g64.norm()) < 1e-12                      # the split restates the oracle's gradient
    return g_dec, basis


def _ref(key, loss_fn, l1_parts, sd, taps, criterion, image):
    if key not in _REFS:
        x, gt = images(*image)
        l32, g32 = _loss_and_grad(lambda a, b: loss_fn(_cast(sd, torch.float32), a, b), x, gt, torch.float32)
        l64, g64 = _loss_and_grad(lambda a, b: loss_fn(_cast(sd, torch.float64), a, b), x, gt, torch.float64)
        decided = basis = allowed = None
        if criterion == "l1":
            pre, act, allowed = l1_parts
            decided, basis = _l1_split(pre, act, sd, taps, x, gt, g64)
            allowed = torch.tensor(allowed, dtype=torch.float64)
        _REFS[key] = Ref(l32, g32, l64, g64, decided, basis, allowed)
    return _REFS[key]


def vgg_ref(taps, criterion="mse", seed=VGG_SEED, biased=True, image=(IMAGE_SEED, B, H, W)):
    """Ref of oracle.vgg.content_loss; cached, do not write into the result."""
    import torch.nn.functional as F
    from oracle import vgg as ovgg

    def pre(sd, a):                 # features.<K - 1> is the conv whose ReLU is features.<K>
        f = ovgg.vgg_features(sd, a, tuple(t - 1 for t in taps))
        return {t: f[t - 1] for t in taps}
    key = ("vgg", tuple(sorted(taps.items())), criterion, seed, biased, image)
    return _ref(key, lambda sd, a, b: ovgg.content_loss(sd, a, b, layers(taps), criterion), (pre, F.relu, (-1.0, 0.0, 1.0)),
                vgg_state(seed, biased), taps, criterion, image)


def disc_ref(taps, criterion="mse", seed=DISC_SEED, image=(IMAGE_SEED, B, H, W)):
    """Ref of oracle.model.disc_content_loss; cached, do not write into the result."""
    import torch.nn.functional as F
    from oracle import model as om

    def pre(sd, a):                 # LeakyReLU is invertible: its input from the oracle's tap (autograd passes through both)
        mean = torch.tensor(om.IMAGENET_MEAN, dtype=a.dtype).view(1, 3, 1, 1)
        std = torch.tensor(om.IMAGENET_STD, dtype=a.dtype).view(1, 3, 1, 1)
        f = om.discriminator_features(sd, (a - mean) / std, set(taps))
        return {t: torch.where(f[t] >= 0, f[t], f[t] / 0.2) for t in taps}
    key = ("disc", tuple(sorted(taps.items())), criterion, seed, image)
    return _ref(key, lambda sd, a, b: om.disc_content_loss(sd, a, b, layers(taps), criterion),
                (pre, lambda z: F.leaky_relu(z, 0.2), (-1.0, -0.2, 0.0, 0.2, 1.0)), disc_state(seed), taps, criterion, image)


def rel_loss_err(loss, ref):
    return abs(float(loss) - float(ref)) / abs(float(ref))


def vgg_mask_ref(taps, seed=VGG_SEED, biased=True, image=(IMAGE_SEED, B, H, W)):
    """A measuring aid for the MSE criterion at sizes where ReLU masks INSIDE the stack become undecidable ("Feature criteria
    against fp64"): the Ref of vgg_ref(taps, "mse") with a basis over every SR pre-activation z_i, at any conv, within delta of zero
    (delta per layer as above).  Flipping the mask of such an element moves d loss / d sr by exactly
    +- (d loss / d relu(z_i)) * d z_i / d sr, since relu(z_i) ~ 0 either way; grad_err fits a coefficient in {-1, 0, +1} to each."""
    from oracle import vgg as ovgg
    key = ("vgg-masks", tuple(sorted(taps.items())), seed, biased, image)
    if key in _REFS:
        return _REFS[key]
    plain = vgg_ref(taps, "mse", seed, biased, image)
    sd = vgg_state(seed, biased)
    sd64, sd32 = _cast(sd, torch.float64), _cast(sd, torch.float32)
    x, gt = images(*image)
    convs = [i for i, kind, _, _ in ovgg.layer_list(max(taps)) if kind == "conv"]
    x64 = x.double().requires_grad_(True)
    f = ovgg.vgg_features(sd64, x64, tuple(convs) + tuple(c + 1 for c in convs))
    fg = ovgg.vgg_features(sd64, gt.double(), tuple(taps))
    with torch.no_grad():
        z32 = ovgg.vgg_features(sd32, x, tuple(convs))
    loss = sum(w * torch.nn.functional.mse_loss(f[t], fg[t]) for t, w in taps.items())
    g_act = torch.autograd.grad(loss, [f[c + 1] for c in convs], retain_graph=True)
    rows = []
    for c, ga in zip(convs, g_act):
        z = f[c].flatten()
        delta = 3.0 * float((z32[c].flatten().double() - z.detach()).abs().max())
        for i in (z.detach().abs() < delta).nonzero().flatten().tolist():
            rows.append(float(ga.flatten()[i]) * torch.autograd.grad(z[i], x64, retain_graph=True)[0].flatten())
    basis = torch.stack(rows) if rows else None
    _REFS[key] = Ref(plain.loss32, plain.grad32, plain.loss64, plain.grad64, plain.grad64, basis, torch.tensor((-1.0, 0.0, 1.0), dtype=torch.float64))
    return _REFS[key]
