"""Training state: everything a run needs to continue as if it had never stopped, in one file.

``g_last.pth`` / ``d_last.pth`` hold weights only.  ``state_last.pth`` (written by the drivers after every epoch unless
``EXP.SAVE_STATE`` is off) adds what a continued run needs to be the SAME run: both optimizers' state (Adam moments and step
counters, i.e. the bias correction), both LR schedulers, the averaged generator (``SOLVER.G_EMA_DECAY``), the best validation
values, warmup's batch counter and the CPU / device RNG streams - plus a fingerprint of the settings that must agree.  With
gradient clipping or the non-finite guard on (``SOLVER.G_GRAD_CLIP`` / ``D_GRAD_CLIP`` / ``SKIP_NONFINITE``) a ``"clip"`` entry
carries their cumulative counters per network; a file without it resumes with the counters at zero.

The file is one ``torch.save`` of tensors and plain Python values (loads with ``weights_only=True`` like every checkpoint of the
project), written to a temporary name in the target's directory and moved into place with ``os.replace``: a run killed mid-write
leaves the previous state intact.

    d(t) of the average (optim.FlatAdam / csrc/optim.hip) is restated here as ``ema_decay_at`` for hosts and tests.
"""
from __future__ import annotations

import os
import tempfile
from collections import Counter

import torch

from . import dist as sdist

FORMAT_VERSION = 1
STATE_FILE = "state_last.pth"

# what must agree between the run that wrote a state and the run that continues it
FINGERPRINT_FIELDS = ("g_n_channel", "g_n_rcb", "d_n_channel", "upscale_factor", "batch_size", "world_size", "g_ema")


def ema_decay_at(t, ema_decay, ema_warmup=True):
    """The decay the flat Adam kernel applies to the parameter average at Adam step t (1 at the first update)."""
    t = float(t)
    return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if ema_warmup else float(ema_decay)


def fingerprint(config, world_size=None):
    return {
        "g_n_channel": int(config.MODEL.G_N_CHANNEL),
        "g_n_rcb": int(config.MODEL.G_N_RCB),
        "d_n_channel": int(config.MODEL.D_N_CHANNEL),
        "upscale_factor": int(config.DATA.UPSCALE_FACTOR),
        "batch_size": int(config.DATA.BATCH_SIZE),
        "world_size": int(sdist.world_size() if world_size is None else world_size),
        "g_ema": bool(float(config.SOLVER.get("G_EMA_DECAY", 0.0)) > 0.0),
    }


def check_fingerprint(state, config, world_size=None, path="training state"):
    """Raise, naming the field, when `state` was written by a run this one cannot continue."""
    if state.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{path}: format_version is {state.get('format_version')!r}, this code reads {FORMAT_VERSION}")
    have, want = state["fingerprint"], fingerprint(config, world_size)
    for field in FINGERPRINT_FIELDS:
        if have.get(field) != want[field]:
            raise ValueError(f"{path}: cannot resume, {field} is {have.get(field)!r} in the file and {want[field]!r} in this run")


def _plain(obj):
    """Containers weights_only loading does not know (a scheduler's Counter of milestones) as plain dicts / lists."""
    if isinstance(obj, Counter):
        return {k: int(v) for k, v in obj.items()}
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    return obj


def scheduler_state(sched):
    return None if sched is None else _plain(sched.state_dict())


def load_scheduler_state(sched, sd):
    """sched.load_state_dict with the containers _plain flattened put back (MultiStepLR bisects a Counter)."""
    sd = dict(sd)
    for k, v in sd.items():
        if isinstance(getattr(sched, k, None), Counter):
            sd[k] = Counter(v)
    sched.load_state_dict(sd)


def rng_state(device=None):
    out = {"cpu": torch.get_rng_state(), "cuda": None}
    if device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available():
        out["cuda"] = torch.cuda.get_rng_state(torch.device(device))
    return out


def restore_rng(rng, device=None):
    torch.set_rng_state(rng["cpu"].cpu())
    if rng.get("cuda") is not None and device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available():
        torch.cuda.set_rng_state(rng["cuda"].cpu(), torch.device(device))


def atomic_save(obj, path):
    """torch.save to a temporary file beside `path`, then os.replace: `path` is either the old file or the complete new one."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=d)
    os.close(fd)
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def save_training_state(path, *, epoch, generator, g_opt, g_sched, discriminator=None, d_opt=None, d_sched=None, g_ema=None,
                        best=(0.0, 0.0), batches_done=0, config, world_size=None, clip=None):
    """epoch: the NEXT epoch to run.  g_ema: the averaged generator (a module) or None.  clip: engine.clip_state() - the counters
    of gradient clipping / the non-finite guard per network, {"G": {...}, "D": {...}} - or None (feature off: no entry)."""
    device = next(generator.parameters()).device
    state = {
        "format_version": FORMAT_VERSION,
        "epoch": int(epoch),
        "generator": generator.state_dict(),
        "discriminator": None if discriminator is None else discriminator.state_dict(),
        "g_opt": g_opt.state_dict(),
        "d_opt": None if d_opt is None else d_opt.state_dict(),
        "g_sched": scheduler_state(g_sched),
        "d_sched": scheduler_state(d_sched),
        "g_ema": None if g_ema is None else g_ema.state_dict(),
        "best_psnr": float(best[0]),
        "best_ssim": float(best[1]),
        "batches_done": int(batches_done),
        "rng": rng_state(device),
        "fingerprint": fingerprint(config, world_size),
    }
    if clip:
        state["clip"] = {str(net): {str(k): int(v) for k, v in c.items()} for net, c in clip.items() if c is not None}
    atomic_save(state, path)


def load_training_state(path, map_location, config=None, world_size=None):
    """The dict save_training_state wrote.  With `config`: checked against this run's fingerprint (ValueError naming the field)."""
    state = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(state, dict) or "format_version" not in state:
        raise ValueError(f"{path}: not a training-state file")
    if config is not None:
        check_fingerprint(state, config, world_size, path=str(path))
    return state


def resume_path(config):
    """EXP.RESUME as a path, or None for a fresh start ("" and "auto" without a file)."""
    r = config.EXP.get("RESUME", "") or ""
    if r == "auto":
        p = os.path.join("results", config.EXP.NAME, STATE_FILE)
        return p if os.path.exists(p) else None
    return r or None


def load_resume(config, world_size=None):
    """The state EXP.RESUME names (checked against this run), or None; config.EXP.START_EPOCH is set from it."""
    path = resume_path(config)
    if path is None:
        return None
    state = load_training_state(path, config.DEVICE, config=config, world_size=world_size)
    config.EXP.START_EPOCH = state["epoch"]
    return state
