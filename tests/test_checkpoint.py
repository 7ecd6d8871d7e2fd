"""CPU: the training-state file (srganst/checkpoint.py) - round trip, weights_only loading, atomic replacement, the fingerprint
that guards a resume, EXP.RESUME = "auto", and the host restatement of the average's decay d(t)."""
import os
from collections import Counter

import pytest
import torch

from ema_refs import decay_at, equal_tree


def _cfg():
    from srganst.config import Config
    cfg = Config()
    cfg.DEVICE = "cpu"
    cfg.EXP.NAME = "ckpt"
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 8, 1, 4
    cfg.DATA.BATCH_SIZE = 4
    cfg.SOLVER.G_EMA_DECAY = 0.999
    return cfg


def _run(cfg, steps=3):
    """CPU modules with stock torch.optim.Adam + MultiStepLR after a few steps on random gradients (moments, step counters and
    the LR drop at the milestone are all alive)."""
    from srganst.model import Discriminator, Generator
    torch.manual_seed(3)
    G, D, E = Generator(cfg), Discriminator(cfg), Generator(cfg)
    g_opt = torch.optim.Adam(G.parameters(), lr=1e-3, eps=1e-4)
    d_opt = torch.optim.Adam(D.parameters(), lr=2e-3, eps=1e-4)
    g_sched = torch.optim.lr_scheduler.MultiStepLR(g_opt, milestones=[2], gamma=0.5)
    d_sched = torch.optim.lr_scheduler.MultiStepLR(d_opt, milestones=[2], gamma=0.5)
    for _ in range(steps):
        for m, o, s in ((G, g_opt, g_sched), (D, d_opt, d_sched)):
            for p in m.parameters():
                p.grad = torch.randn_like(p)
            o.step()
            s.step()
    return G, D, E, g_opt, d_opt, g_sched, d_sched


def _save(path, cfg, run, **kw):
    from srganst import checkpoint
    G, D, E, g_opt, d_opt, g_sched, d_sched = run
    args = dict(epoch=3, generator=G, g_opt=g_opt, g_sched=g_sched, discriminator=D, d_opt=d_opt, d_sched=d_sched, g_ema=E,
                best=(27.25, 0.8125), batches_done=15, config=cfg, world_size=1)
    args.update(kw)
    checkpoint.save_training_state(path, **args)


def test_round_trip_restores_everything(tmp_path):
    from srganst import checkpoint
    cfg = _cfg()
    run = _run(cfg)
    G, D, E, g_opt, d_opt, g_sched, d_sched = run
    path = str(tmp_path / "state_last.pth")
    _save(path, cfg, run)
    after_save = torch.rand(5)
    torch.manual_seed(12345)          # the streams move on ...
    torch.rand(7)
    st = checkpoint.load_training_state(path, "cpu", config=cfg, world_size=1)
    assert st["format_version"] == checkpoint.FORMAT_VERSION
    assert st["epoch"] == 3 and st["best_psnr"] == 27.25 and st["best_ssim"] == 0.8125 and st["batches_done"] == 15
    assert equal_tree(st["generator"], G.state_dict()) and list(st["generator"].keys()) == list(G.state_dict().keys())
    assert equal_tree(st["discriminator"], D.state_dict())
    assert equal_tree(st["g_ema"], E.state_dict())
    assert equal_tree(st["g_opt"], g_opt.state_dict()) and equal_tree(st["d_opt"], d_opt.state_dict())
    assert float(st["g_opt"]["param_groups"][0]["lr"]) == 0.5e-3          # the milestone has passed
    # the schedulers: into fresh ones, whose state then equals the originals' (MultiStepLR's Counter of milestones included)
    from srganst.model import Generator
    G2 = Generator(cfg)
    o2 = torch.optim.Adam(G2.parameters(), lr=1e-3, eps=1e-4)
    s2 = torch.optim.lr_scheduler.MultiStepLR(o2, milestones=[2], gamma=0.5)
    o2.load_state_dict(st["g_opt"])
    checkpoint.load_scheduler_state(s2, st["g_sched"])
    assert isinstance(s2.milestones, Counter) and s2.state_dict() == g_sched.state_dict()
    assert s2.last_epoch == 3 and s2.get_last_lr() == g_sched.get_last_lr()
    # ... and come back: the next draw is the draw that followed the save
    checkpoint.restore_rng(st["rng"], "cpu")
    assert torch.equal(torch.rand(5), after_save)


def test_state_file_loads_with_weights_only(tmp_path):
    cfg = _cfg()
    path = str(tmp_path / "state_last.pth")
    _save(path, cfg, _run(cfg, steps=1))
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert {"format_version", "epoch", "generator", "discriminator", "g_opt", "d_opt", "g_sched", "d_sched", "g_ema", "best_psnr",
            "best_ssim", "batches_done", "rng", "fingerprint"} == set(st)
    assert st["rng"]["cpu"].dtype == torch.uint8


def test_generator_only_state(tmp_path):
    """warmup(): no discriminator, no scheduler, no average."""
    from srganst import checkpoint
    cfg = _cfg()
    cfg.SOLVER.G_EMA_DECAY = 0.0
    path = str(tmp_path / "state_last.pth")
    _save(path, cfg, _run(cfg, steps=1), discriminator=None, d_opt=None, d_sched=None, g_sched=None, g_ema=None)
    st = checkpoint.load_training_state(path, "cpu", config=cfg, world_size=1)
    assert st["discriminator"] is None and st["d_opt"] is None and st["g_sched"] is None and st["g_ema"] is None


def test_failed_write_leaves_previous_state_intact(tmp_path, monkeypatch):
    cfg = _cfg()
    run = _run(cfg, steps=1)
    path = tmp_path / "state_last.pth"
    _save(str(path), cfg, run)
    before = path.read_bytes()
    real_save = torch.save

    def dying_save(obj, f, *a, **k):
        with open(f, "wb") as fh:          # the temporary file exists and is half written when the run dies
            fh.write(b"partial")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(OSError, match="disk full"):
        _save(str(path), cfg, run, epoch=4)
    monkeypatch.setattr(torch, "save", real_save)
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["state_last.pth"]


_ALTER = {
    "g_n_channel": lambda c: c.MODEL.__setitem__("G_N_CHANNEL", 16),
    "g_n_rcb": lambda c: c.MODEL.__setitem__("G_N_RCB", 2),
    "d_n_channel": lambda c: c.MODEL.__setitem__("D_N_CHANNEL", 8),
    "upscale_factor": lambda c: c.DATA.__setitem__("UPSCALE_FACTOR", 2),
    "batch_size": lambda c: c.DATA.__setitem__("BATCH_SIZE", 8),
    "world_size": None,
    "g_ema": lambda c: c.SOLVER.__setitem__("G_EMA_DECAY", 0.0),
}


@pytest.fixture(scope="module")
def saved_state(tmp_path_factory):
    cfg = _cfg()
    path = str(tmp_path_factory.mktemp("fp") / "state_last.pth")
    _save(path, cfg, _run(cfg, steps=1))
    return path


@pytest.mark.parametrize("field", list(_ALTER))
def test_fingerprint_mismatch_names_the_field(saved_state, field):
    from srganst import checkpoint
    assert set(_ALTER) == set(checkpoint.FINGERPRINT_FIELDS)
    cfg = _cfg()
    checkpoint.load_training_state(saved_state, "cpu", config=cfg, world_size=1)          # unaltered: accepted
    world = 1
    if _ALTER[field] is None:
        world = 2
    else:
        _ALTER[field](cfg)
    with pytest.raises(ValueError, match=field):
        checkpoint.load_training_state(saved_state, "cpu", config=cfg, world_size=world)


def test_resume_auto(tmp_path, monkeypatch):
    from srganst import checkpoint
    monkeypatch.chdir(tmp_path)
    cfg = _cfg()
    assert cfg.EXP.RESUME == "" and cfg.EXP.SAVE_STATE is True
    assert checkpoint.load_resume(cfg, 1) is None                         # off
    cfg.EXP.RESUME = "auto"
    assert checkpoint.resume_path(cfg) is None and checkpoint.load_resume(cfg, 1) is None      # no file: a fresh start
    assert cfg.EXP.START_EPOCH == 0
    _save("results/ckpt/state_last.pth", cfg, _run(cfg, steps=1))
    assert checkpoint.resume_path(cfg) == os.path.join("results", "ckpt", "state_last.pth")
    st = checkpoint.load_resume(cfg, 1)
    assert st["epoch"] == 3 and cfg.EXP.START_EPOCH == 3                  # the next epoch to run
    cfg.EXP.RESUME = "results/elsewhere.pth"                             # a path that does not exist is an error, not a fresh start
    with pytest.raises(FileNotFoundError):
        checkpoint.load_resume(cfg, 1)


@pytest.mark.parametrize("t,expect_warm", [(1, 2 / 11), (2, 3 / 12), (9, 10 / 19), (10 ** 4, 0.999)])
def test_decay_restatement(t, expect_warm):
    from srganst.checkpoint import ema_decay_at
    assert ema_decay_at(t, 0.999, True) == decay_at(t, 0.999, True) == expect_warm
    assert ema_decay_at(t, 0.999, False) == decay_at(t, 0.999, False) == 0.999
