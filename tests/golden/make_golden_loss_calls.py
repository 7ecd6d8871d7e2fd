"""Records what the criteria ask of the library -> tests/golden/loss_calls.json.

Needs the GPU.  Per case: every call of an entry whose name starts with one of PREFIXES, in order, with its arguments (integers and
floats as they are, pointers as null / non-null by _abi.SIGNATURES, the weights of sst_weighted_sum read back from its float array),
the loss and each weighted value as float.hex, and the SHA-256 of the bytes of sr.grad after (3 * total).backward().  The kernels are
bit-reproducible from run to run, so a replay is compared for equality.  Only names that outlive a rewrite of the host side are used
(the public criteria, criterion_sum, engine._criterion_total, the two module switches, _abi).  Record it from a checkout of the commit
whose calls are to be preserved:

    python tests/golden/make_golden_loss_calls.py

tests/test_loss_calls_gpu.py replays it against the tree under test.
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "loss_calls.json")

PREFIXES = ("sst_st_", "sst_ssim_", "sst_freq_", "sst_bp_", "sst_pixel_loss_", "sst_feat_loss_", "sst_bb", "sst_bicubic", "sst_weighted_sum")
# two 32-px tiles in each direction, both partial in the last row and column, above SSIM's 11-px minimum
B, H, W = 2, 40, 36
SEED = 20
GRAD_SEED = 3.0                       # (3 * total).backward(): a non-unit scale_dev
CONTENT_SHAPE = (3, 32, 48)           # the smallest configuration of tests/test_content_losses_fp64_gpu.py
VGG_TAPS = {1: 0.3, 3: 0.7}
DISC_TAPS = {1: 0.4, 4: 0.6}


class _Recorder:
    """Stands in for _abi._lib: hands every entry through, and notes the calls of the PREFIXES entries."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        from srganst import _abi
        fn = getattr(self._lib, name)
        if not name.startswith(PREFIXES):
            return fn
        argtypes = _abi.SIGNATURES[name][1]

        def recorded(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            row = [name] + [_plain(a, t) for a, t in zip(args, argtypes)]
            if name == "sst_weighted_sum":
                row.append([float(args[1][i]) for i in range(args[2])])
            self._calls.append(row)
            return fn(*args)
        return recorded


def _plain(a, argtype):
    if argtype in (ctypes.c_int, ctypes.c_int64):
        return int(a)
    if argtype in (ctypes.c_float, ctypes.c_double):
        return float(a)
    return "null" if a is None or (isinstance(a, int) and a == 0) else "ptr"


@contextlib.contextmanager
def _recording(calls, fuse, force_general):
    from srganst import _abi
    from srganst import loss as L
    saved = _abi._lib, L.FUSE_PIXEL_INTO_ST, L.ST_FORCE_GENERAL
    try:
        _abi._lib = _Recorder(_abi.lib(), calls)
        L.FUSE_PIXEL_INTO_ST, L.ST_FORCE_GENERAL = fuse, force_general
        yield
    finally:
        _abi._lib, L.FUSE_PIXEL_INTO_ST, L.ST_FORCE_GENERAL = saved


def images(b=B, h=H, w=W, seed=SEED):
    """-> (sr, gt) on the CPU: gt uniform in [0, 1], sr = (gt + 0.1 * randn).clamp(0, 1)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(b, 3, h, w, generator=g)
    return (gt + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1), gt


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _hex(t):
    return float(t.detach()).hex()


def step(fn, shape=(B, H, W), mode="grad", fuse=True, force_general=False, extra=None, second=None, scale=1.0):
    """One recorded call of fn(sr, gt) -> total or (total, {name: value} / [values]).  mode: "grad", "no_grad" (under
    torch.no_grad()) or "no_requires" (sr does not require a gradient).  second: gt on the device -> what fn gets in gt's place (made
    before the recording starts); extra may take (sr, that second argument).  scale: what the images are multiplied by (255: the
    0..255 scale)."""
    import torch
    sr, gt = images(*shape)
    if scale != 1.0:
        sr, gt = sr * scale, gt * scale
    sr = sr.cuda().requires_grad_(mode != "no_requires")
    gt = gt.cuda()
    if second is not None:
        gt = second(gt)
    calls = []
    with _recording(calls, fuse, force_general):
        with torch.no_grad() if mode == "no_grad" else contextlib.nullcontext():
            out = fn(sr, gt)
        total, values = out if isinstance(out, tuple) else (out, [])
        if mode == "grad":
            (GRAD_SEED * total).backward()
        torch.cuda.synchronize()
    assert (mode == "grad") == total.requires_grad, (mode, total.requires_grad)
    if isinstance(values, dict):
        values = OrderedDict((k, _hex(v)) for k, v in values.items())
    else:
        values = [_hex(v) for v in values]
    rec = {"calls": calls, "loss": _hex(total), "values": values, "grad": _sha(sr.grad) if mode == "grad" else None}
    if extra is not None:
        rec.update(extra(sr.detach(), gt) if second is not None else extra())
    return rec


def _config():
    from srganst.config import Config
    cfg = Config()
    cfg.DEVICE = "cuda:0"
    cfg.MODEL.G_LOSS.VGG19_LAYERS = {f"features.{k}": w for k, w in VGG_TAPS.items()}
    cfg.MODEL.G_LOSS.DISC_FEATURES_LOSS_LAYERS = {f"features.{k}": w for k, w in DISC_TAPS.items()}
    return cfg


def cases():
    """name -> function() -> [one record per recorded call].  A function builds its criteria afresh, so the cases are independent of
    each other and of their order."""
    import torch
    from srganst import engine
    from srganst import loss as L
    ST = L.StructureTensorLoss
    out = OrderedDict()

    def alone(name, make, **kw):
        out[name] = lambda: [step(make(), **kw)]

    alone("MSE", L.MSELoss)
    alone("L1", L.L1Loss)
    alone("ST(0.5,2)", lambda: ST(0.5, 2.0))                                   # the two tile builds: radii (2, 8) and (4, 10)
    alone("ST(1,2.5)", lambda: ST(1.0, 2.5))
    alone("ST(1.5,3)", lambda: ST(1.5, 3.0))                                   # the general route, radii (6, 12)
    alone("ST(0.5,2) forced general", lambda: ST(0.5, 2.0), force_general=True)
    alone("ST(0.5,2) normalize=False", lambda: ST(0.5, 2.0, normalize=False))

    def ssim(channel):
        def run():
            crit = L.SSIMLoss(channel)
            return [step(crit, mode=m) for m in ("grad", "no_grad", "no_requires")]
        return run
    out["SSIM(y): grad, no_grad, no requires_grad"] = ssim("y")
    out["SSIM(rgb): grad, no_grad, no requires_grad"] = ssim("rgb")

    def summed(name, make, weights, **kw):
        def run():
            terms = make()
            return [step(lambda sr, gt: L.criterion_sum(sr, gt, terms, weights), **kw)]
        out[name] = run

    for fuse in (True, False):
        tag = "" if fuse else " unfused"
        summed("sum[MSE, ST(0.5,2)]" + tag, lambda: [L.MSELoss(), ST(0.5, 2.0)], [1.0, 1 / 3], fuse=fuse)
        summed("sum[ST(0.5,2), L1]" + tag, lambda: [ST(0.5, 2.0), L.L1Loss()], [0.25, 2.0], fuse=fuse)
    summed("sum[L1, ST(1.5,3)]", lambda: [L.L1Loss(), ST(1.5, 3.0)], [1.0, 1 / 3])
    summed("sum[ST(1.5,3), MSE]", lambda: [ST(1.5, 3.0), L.MSELoss()], [0.5, 1.5])
    summed("sum[MSE]", lambda: [L.MSELoss()], [0.7])
    summed("sum[ST(0.5,2)]", lambda: [ST(0.5, 2.0)], [1 / 3])
    summed("sum[MSE, L1]", lambda: [L.MSELoss(), L.L1Loss()], [1.0, 0.5])
    summed("sum[ST(0.5,2), ST(1,2.5), MSE]", lambda: [ST(0.5, 2.0), ST(1.0, 2.5), L.MSELoss()], [1 / 3, 0.2, 1.0])
    summed("sum[MSE, ST(0.5,2)] forced general", lambda: [L.MSELoss(), ST(0.5, 2.0)], [1.0, 1 / 3], force_general=True)

    def reused(make, weights, **kw):
        """Twice at B = 2 (the second call finds its workspace), at B = 1 (the key changes), and at B = 2 again."""
        def run():
            terms = make()
            fn = lambda sr, gt: L.criterion_sum(sr, gt, terms, weights)
            return [step(fn, shape=s, **kw) for s in ((B, H, W), (B, H, W), (1, H, W), (B, H, W))]
        return run
    out["sum[MSE, ST(0.5,2)] x2, B=1, B=2"] = reused(lambda: [L.MSELoss(), ST(0.5, 2.0)], [1.0, 1 / 3])
    out["sum[L1, ST(0.5,2)] unfused x2, B=1, B=2"] = reused(lambda: [L.L1Loss(), ST(0.5, 2.0)], [1.0, 1 / 3], fuse=False)
    out["sum[ST(1.5,3), MSE] x2, B=1, B=2"] = reused(lambda: [ST(1.5, 3.0), L.MSELoss()], [0.5, 1.5])

    def total():
        crits = OrderedDict([("Pixel", L.MSELoss()), ("ST", ST(0.5, 2.0)), ("SSIM", L.SSIMLoss("y"))])
        weights = {"Pixel": 1.0, "ST": 1 / 3, "SSIM": 0.1}
        return [step(lambda sr, gt: engine._criterion_total(sr, gt, crits, weights))]
    out["engine._criterion_total{MSE, ST(0.5,2), SSIM(y)}"] = total

    def content(kind):
        def run():
            torch.manual_seed(5)                                             # the fresh discriminator's initialisation
            mod = L.ContentLossVGG(_config(), allow_random=True) if kind == "vgg" else L.ContentLossDiscriminator(_config())
            return [step(mod, shape=CONTENT_SHAPE)]
        return run
    out["ContentLossVGG, taps 1 and 3"] = content("vgg")
    out["ContentLossDiscriminator, taps 1 and 4"] = content("disc")

    def patch(make, side):
        def run():
            crit = make()
            return [step(crit, shape=(B, side, side), extra=lambda: {"last_index": _sha(crit.last_index)})]
        return run
    out["BestBuddyLoss 48 px (register path)"] = patch(L.BestBuddyLoss, 48)
    out["BestBuddyLoss 42 px (table path)"] = patch(L.BestBuddyLoss, 42)
    out["GramLoss 48 px"] = patch(L.GramLoss, 48)
    out["PatchwiseStructureTensorLoss 48 px"] = patch(L.PatchwiseStructureTensorLoss, 48)

    # --- the Fourier-domain and the back-projection criteria (recorded before their reduction epilogue moved into csrc/common.h)
    Freq, BP = L.FocalFrequencyLoss, L.BackProjectionLoss

    def modes(make):
        def run():
            crit = make()
            return [step(crit, mode=m) for m in ("grad", "no_grad", "no_requires")]
        return run
    out["Frequency(1.0): grad, no_grad, no requires_grad"] = modes(lambda: Freq(1.0))
    out["Frequency(0.0): grad, no_grad, no requires_grad"] = modes(lambda: Freq(0.0))
    for scale in L.BP_SCALES:                                                  # 40 x 36 is not a multiple of 8
        for crit in ("l1", "mse"):
            alone(f"BP({scale},{crit})", lambda scale=scale, crit=crit: BP(scale, crit))
    alone("BP(4,l1) round_target=False", lambda: BP(4, "l1", round_target=False))

    def lr_of(scale):
        from srganst.bicubic import Bicubic
        return lambda gt: Bicubic()(gt, 1.0 / scale)

    def lr_consistency(sr, lr):
        from srganst import metrics
        return {"lr_consistency": _sha(metrics.lr_consistency(sr, lr, 4))}
    out["BP(4,l1) target=lr, metrics.lr_consistency"] = lambda: [step(BP(4, "l1", target="lr"), second=lr_of(4), extra=lr_consistency)]

    def total_new():
        crits = OrderedDict([("Pixel", L.MSELoss()), ("Frequency", Freq()), ("BackProjection", BP(4))])
        weights = {"Pixel": 1.0, "Frequency": 1.0, "BackProjection": 0.1}
        return [step(lambda sr, gt: engine._criterion_total(sr, gt, crits, weights))]
    out["engine._criterion_total{MSE, Frequency, BackProjection}"] = total_new

    def reused_alone(make):
        """reused() for a criterion outside criterion_sum: the B = 1 call re-keys its workspace and its scratch."""
        def run():
            crit = make()
            return [step(crit, shape=s) for s in ((B, H, W), (B, H, W), (1, H, W), (B, H, W))]
        return run
    out["SSIM(y) x2, B=1, B=2"] = reused_alone(lambda: L.SSIMLoss("y"))
    out["Frequency(1.0) x2, B=1, B=2"] = reused_alone(Freq)
    out["BP(4,l1) x2, B=1, B=2"] = reused_alone(lambda: BP(4))

    # more workgroups than the last arriver has threads (256), and no multiple of them: its strided loop over the partials runs a
    # second, ragged pass.  The counts are the entries' own (sst_*_workspace: partial floats / 2).
    for name, make, shape in MANY_PARTIALS:
        alone(f"{name} at {shape}: {many_partials(name)} partials", make, shape=(shape[0], shape[2], shape[3]))

    # --- the structure-tensor family (recorded before its three sources came to share csrc/st_tile.h): the <4,10> tile build, the
    # general route at radii (4, 8) and at its bound (8, 20), normalize=False on 0..255 inputs on either route, the fused pair on
    # the <4,10> build
    for shape in ST_SHAPES:
        at = f" at {list(shape)}"
        alone("ST(1,2.5)" + at, lambda: ST(1.0, 2.5), shape=shape)
        alone("ST(1,2)" + at, lambda: ST(1.0, 2.0), shape=shape)
        alone("ST(2,5)" + at, lambda: ST(2.0, 5.0), shape=shape)
        alone("ST(0.5,2) normalize=False on 0..255" + at, lambda: ST(0.5, 2.0, normalize=False), shape=shape, scale=255.0)
        alone("ST(1,2) normalize=False on 0..255" + at, lambda: ST(1.0, 2.0, normalize=False), shape=shape, scale=255.0)
        summed("sum[L1, ST(1,2.5)]" + at, lambda: [L.L1Loss(), ST(1.0, 2.5)], [1.0, 1 / 3], shape=shape)
    return out


# partial tiles on both axes with W no multiple of 4; smaller than every halo; exactly one tile
ST_SHAPES = ((2, 33, 31), (1, 5, 3), (2, 32, 32))
MANY_PARTIALS = [("SSIM(rgb)", lambda: _loss().SSIMLoss("rgb"), (16, 3, 43, 75)),
                 ("Frequency(1.0)", lambda: _loss().FocalFrequencyLoss(), (43, 3, 48, 48)),
                 ("BP(4,l1)", lambda: _loss().BackProjectionLoss(4), (16, 3, 38, 262))]


def _loss():
    from srganst import loss
    return loss


def many_partials(name):
    """Workgroups of the forward kernel of a MANY_PARTIALS case, asked of the library on the host (no GPU)."""
    from srganst import _abi
    lib, n = _abi.lib(), [ctypes.c_int64() for _ in range(3)]
    r = [ctypes.byref(v) for v in n]
    (b, _, h, w), = [s for k, _, s in MANY_PARTIALS if k == name]
    if name.startswith("SSIM"):
        rc, part = lib.sst_ssim_loss_workspace(b, h, w, 3, r[0], r[1]), n[1]
    elif name.startswith("Frequency"):
        rc, part = lib.sst_freq_loss_workspace(b, h, w, r[0], r[1], r[2]), n[2]
    else:
        rc, part = lib.sst_bp_loss_workspace(b, h, w, 4, r[0], r[1]), n[1]
    assert rc == 0 and part.value % 2 == 0 and part.value // 2 > 256 and (part.value // 2) % 256, (name, rc, part.value)
    return part.value // 2


def record():
    return OrderedDict((name, run()) for name, run in cases().items())


def main():
    recs = record()
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:                 # one line per case: a changed case is one changed line
        f.write('{"shape": %s, "seed": %d, "cases": {\n' % (json.dumps([B, H, W]), SEED))
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(r, separators=(',', ':'))}" for name, r in recs.items()))
        f.write("\n}}\n")
    print({name: [len(s["calls"]) for s in r] for name, r in recs.items()})


if __name__ == "__main__":
    main()
