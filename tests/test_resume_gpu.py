"""GPU: a run continued from its training state (EXP.RESUME, srganst/checkpoint.py) is the run that was never stopped, and the
averaged generator (SOLVER.G_EMA_DECAY) is saved, validated and usable like any generator checkpoint.

Drivers as in tests/test_drivers_gpu.py (16 / 8 channels, 2 blocks, B = 4, 96 px, five steps per epoch).  Bitwise equality is
the bar at this shape: hipGraph replay equals eager bit for bit and no reduction here uses the 64-channel trunk's fp64 atomics."""
import contextlib
import os
import shutil

import pytest
import torch

from ema_refs import equal_tree
from test_drivers_gpu import _Pairs, _cfg as _driver_cfg

pytestmark = pytest.mark.gpu


class _Recorder:
    """Stands in for the drivers' SummaryWriter: keeps the scalars."""

    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[(tag, step)] = value

    def add_text(self, *a, **k):
        pass


@contextlib.contextmanager
def _in_dir(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def _cfg(tmp, name, kind, **exp):
    from srganst.loss import MSELoss, StructureTensorLoss
    cfg = _driver_cfg(str(tmp), name)
    cfg.SOLVER.G_EMA_DECAY = 0.999
    if kind == "warmup":
        cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss(), "ST": StructureTensorLoss()}
        cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0, "ST": 1 / 3}
    else:
        cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
        cfg.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
        cfg.SOLVER.D_UPDATE_INTERVAL = 2
        cfg.SCHEDULER.MILESTONES = [1]          # the learning rate drops between the two epochs
    for k, v in exp.items():
        cfg.EXP[k] = v
    return cfg


def _drive(kind, cfg):
    """One driver call on the synthetic set; returns the scalars it logged."""
    from srganst import train as train_mod, warmup as warmup_mod
    from srganst.dataset import SyntheticImageDataset
    rec = _Recorder()
    mp = pytest.MonkeyPatch()
    mp.setattr(warmup_mod, "_writer", lambda name: rec)
    mp.setattr(train_mod, "_writer", lambda name: rec)
    try:
        fn = warmup_mod.warmup if kind == "warmup" else train_mod.train
        fn(cfg, train_dataset=SyntheticImageDataset(24, hr=96, seed=1), test_dataset=_Pairs(), max_steps_per_epoch=5)
    finally:
        mp.undo()
    return rec.scalars


def _load(name, f):
    return torch.load(os.path.join("results", name, f), map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """For warmup() and train(): run A straight through two epochs, run B one epoch and then resumed for the second."""
    tmp = tmp_path_factory.mktemp("resume")
    out = {"dir": tmp}
    with _in_dir(tmp):
        for kind in ("warmup", "train"):
            out[kind + "_A"] = _drive(kind, _cfg(tmp, kind + "_A", kind, N_EPOCHS=2))
            _drive(kind, _cfg(tmp, kind + "_B", kind, N_EPOCHS=1))
            assert _load(kind + "_B", "state_last.pth")["epoch"] == 1
            if kind == "train":          # run B's weights after its first epoch, for the weights-only restart below
                os.makedirs("kept", exist_ok=True)
                shutil.copy("results/train_B/g_last.pth", "kept/g_epoch1.pth")
            out[kind + "_B"] = _drive(kind, _cfg(tmp, kind + "_B", kind, N_EPOCHS=2, RESUME="auto"))
    return out


def _opt_tensors(state, key):
    sd = state[key]
    return {(i, k): st[k] for i, st in sd["state"].items() for k in ("exp_avg", "exp_avg_sq", "step")}


@pytest.mark.parametrize("kind", ["warmup", "train"])
def test_resumed_run_equals_uninterrupted_run(runs, kind):
    with _in_dir(runs["dir"]):
        a, b = kind + "_A", kind + "_B"
        files = ["g_last.pth", "g_ema_last.pth"] + (["d_last.pth"] if kind == "train" else [])
        for f in files:
            sa, sb = _load(a, f), _load(b, f)
            assert list(sa) == list(sb)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), (f, k)
        assert not equal_tree(_load(a, "g_last.pth"), _load(a, "g_ema_last.pth"))      # the average is not the last iterate
        sa, sb = _load(a, "state_last.pth"), _load(b, "state_last.pth")
        assert sa["epoch"] == sb["epoch"] == 2
        for opt in ("g_opt",) + (("d_opt",) if kind == "train" else ()):
            ta, tb = _opt_tensors(sa, opt), _opt_tensors(sb, opt)
            assert ta.keys() == tb.keys() and len(ta) > 0
            for k in ta:
                assert torch.equal(ta[k], tb[k]), (opt, k)
            lr_a, lr_b = float(sa[opt]["param_groups"][0]["lr"]), float(sb[opt]["param_groups"][0]["lr"])
            assert lr_a == lr_b
            if kind == "train":          # the milestone at 1 has passed: the schedule position came back too
                assert lr_a == pytest.approx(0.5 * 1e-4, rel=1e-6)
        n_steps = {float(v) for (i, k), v in _opt_tensors(sa, "g_opt").items() if k == "step"}
        assert n_steps == {10.0}
        assert sa["best_psnr"] == sb["best_psnr"] and sa["best_ssim"] == sb["best_ssim"] and sa["best_psnr"] > 0
        assert sa["batches_done"] == sb["batches_done"] == (10 if kind == "warmup" else 0)
        assert equal_tree(sa["g_ema"], sb["g_ema"]) and equal_tree(sa["g_sched"], sb["g_sched"])
        assert equal_tree(sa["rng"], sb["rng"])
        # the second epoch logged the same validation values
        assert runs[a][("Test/PSNR", 2)] == runs[b][("Test/PSNR", 2)] and runs[a][("Test/SSIM", 2)] == runs[b][("Test/SSIM", 2)]


def test_weights_only_restart_is_a_different_run(runs):
    """START_EPOCH = 1 on run B's first-epoch weights - all that exists without the training state - gives cold moments, a full
    first step and the learning rate back at its base: it must NOT reproduce run A, or the test above could not tell."""
    tmp = runs["dir"]
    with _in_dir(tmp):
        w = torch.load("kept/g_epoch1.pth", map_location="cpu", weights_only=True)
        cfg = _cfg(tmp, "train_C", "train", N_EPOCHS=2, START_EPOCH=1)
        cfg.MODEL.G_CONTINUE_FROM_WARMUP, cfg.MODEL.G_WARMUP_WEIGHTS = True, "kept/g_epoch1.pth"
        _drive("train", cfg)
        a, c = _load("train_A", "g_last.pth"), _load("train_C", "g_last.pth")
        assert not equal_tree(w, c)                                          # it trained
        assert any(not torch.equal(a[k], c[k]) for k in a if k.endswith("weight"))
        sa, sc = _load("train_A", "state_last.pth"), _load("train_C", "state_last.pth")
        assert {float(v) for (i, k), v in _opt_tensors(sc, "g_opt").items() if k == "step"} == {5.0}      # cold bias correction
        assert not equal_tree(_opt_tensors(sa, "g_opt"), _opt_tensors(sc, "g_opt"))


def test_resume_with_on_device_loader_draws_the_same_batches(tmp_path):
    with _in_dir(tmp_path):
        def cfg(name, **exp):
            c = _cfg(tmp_path, name, "warmup", **exp)
            c.DATA.ON_DEVICE = True
            return c
        _drive("warmup", cfg("dev_A", N_EPOCHS=2))
        _drive("warmup", cfg("dev_B", N_EPOCHS=1))
        _drive("warmup", cfg("dev_B", N_EPOCHS=2, RESUME="auto"))
        a, b = _load("dev_A", "g_last.pth"), _load("dev_B", "g_last.pth")
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert equal_tree(_load("dev_A", "g_ema_last.pth"), _load("dev_B", "g_ema_last.pth"))


def test_averaged_generator_checkpoint_is_a_generator_checkpoint(runs):
    from srganst.model import Generator
    from srganst.upscale import Upscaler, generator_from_checkpoint
    from srganst.utils import load_state_dict
    from srganst.validate import test as run_test
    tmp = runs["dir"]
    with _in_dir(tmp):
        cfg = _cfg(tmp, "train_A", "train")
        sd = _load("train_A", "g_ema_last.pth")
        assert list(sd.keys()) == list(Generator(cfg).state_dict().keys())
        assert int(sd["trunk.0.rcb.1.num_batches_tracked"]) == 10           # G's BatchNorm buffers, copied
        g_sd = _load("train_A", "g_last.pth")
        assert all(torch.equal(sd[k], g_sd[k]) for k in sd if "running_" in k or "num_batches" in k)
        G = load_state_dict(Generator(cfg), sd)
        assert equal_tree(dict(G.state_dict()), dict(sd))
        assert os.path.exists("results/train_A/g_ema_best.pth") and os.path.exists("results/train_A/g_best.pth")
        # G_EMA_VALIDATE (default on): the PSNR / SSIM train() recorded for the last epoch are the averaged generator's
        psnr_ema, ssim_ema = run_test(cfg, save_images=False, g_path="results/train_A/g_ema_last.pth", dataset=_Pairs())
        psnr_raw, _ = run_test(cfg, save_images=False, g_path="results/train_A/g_last.pth", dataset=_Pairs())
        logged = runs["train_A"]
        assert logged[("Test/PSNR", 2)] == psnr_ema and logged[("Test/SSIM", 2)] == ssim_ema
        assert logged[("Test/PSNR", 2)] != psnr_raw
        # with no g_path validate.test() prefers the averaged generator's best
        best = _load("train_A", "state_last.pth")
        psnr_best, ssim_best = run_test(cfg, save_images=False, dataset=_Pairs())
        assert (psnr_best, ssim_best) == (best["best_psnr"], best["best_ssim"])
        up = Upscaler(generator_from_checkpoint("results/train_A/g_ema_last.pth", "cuda"), tile=32)
        out = up(torch.rand(1, 3, 24, 40, generator=torch.Generator().manual_seed(4)).cuda())
        assert out.shape == (1, 3, 96, 160) and bool(torch.isfinite(out).all())


def test_everything_off_writes_the_files_it_always_wrote(tmp_path):
    with _in_dir(tmp_path):
        for kind, want in (("warmup", {"g_last.pth", "g_best.pth"}),
                           ("train", {"g_last.pth", "d_last.pth", "g_best.pth", "d_best.pth"})):
            cfg = _cfg(tmp_path, "off_" + kind, kind, N_EPOCHS=1, SAVE_STATE=False)
            cfg.SOLVER.G_EMA_DECAY = 0.0
            _drive(kind, cfg)
            assert set(os.listdir("results/off_" + kind)) == want
