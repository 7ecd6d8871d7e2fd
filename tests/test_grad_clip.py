"""CPU: global gradient-norm clipping and the non-finite guard of the flat Adam - the job table of the norm reduction
(optim.norm_jobs), the fp64 restatement (tests/clip_refs.py) against torch's own clip_grad_norm_ + Adam, the host-side refusals
of the two new entry points (they return before any launch, so they are safe without a GPU), the config keys and the "clip"
entry of the training state."""
import ctypes

import pytest
import torch

from clip_refs import clipped_adam_step_ref, coef_ref
from test_checkpoint import _cfg as _ckpt_cfg, _run as _ckpt_run, _save as _ckpt_save
from test_optim_gpu import _Net


def _grads_cpu(net, step):
    """test_optim_gpu._grads without the copy to the device: the same draws, the same scales (0.1, 1, 10 by turns)."""
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(p.shape, generator=g) * (10.0 ** (step % 3 - 1)) for p in net.parameters()]


def _layouts(chunk):
    from srganst import ops
    params = list(_Net().parameters())
    offs, total = ops.flat_layout(params)
    numels = [p.numel() for p in params]
    assert 1 in numels and 3 in numels
    yield "net", offs, numels, total
    for name, n in (("sixteen", 16), ("chunk", chunk), ("chunk_plus_one", chunk + 1)):
        # a 3-element parameter in front, so that the slot under test starts at 16 and a pad follows the first one
        sizes = [3, n, 5]
        o, t = ops.flat_layout([torch.empty(k) for k in sizes])
        yield name, o, sizes, t


@pytest.mark.parametrize("chunk", [64, 8192])
def test_norm_jobs_cover_every_parameter_element_once_and_no_pad(chunk):
    from srganst.optim import NORM_CHUNK, norm_jobs
    assert NORM_CHUNK == 8192
    for name, offs, numels, total in _layouts(chunk):
        jobs = norm_jobs(offs, numels, chunk)
        hits = torch.zeros(total, dtype=torch.int64)
        for start, count in jobs:
            assert 0 < count <= chunk and 0 <= start and start + count <= total, (name, start, count)
            hits[start:start + count] += 1
        want = torch.zeros(total, dtype=torch.int64)
        for o, n in zip(offs, numels):
            want[o:o + n] = 1
        assert total > sum(numels)                                     # the layout has pad words
        assert torch.equal(hits, want), name
        if name == "chunk_plus_one":
            assert (offs[1] + chunk, 1) in jobs                        # the second job of that slot has one element
            assert (offs[1], chunk) in jobs
        if name == "chunk":
            assert [j for j in jobs if j[0] >= offs[1] and j[0] < offs[2]] == [(offs[1], chunk)]
    assert norm_jobs([0], [0], chunk) == []
    with pytest.raises(ValueError):
        norm_jobs([0], [4], 0)


def test_restatement_against_torch_clip_and_adam():
    """Six steps of test_optim_gpu's gradients in fp64 on the CPU: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam against
    clip_refs.  The gradient norms go 0.1x, 1x, 10x by turns (about 12.6, 126, 1260), so max_norm = 50 clips four steps of six."""
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01)
    max_norm = 50.0
    net = _Net().double()
    opt = torch.optim.Adam(net.parameters(), **kw)
    p = [x.detach().clone() for x in net.parameters()]
    m, v, t = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p], 0
    clipped = []
    for step in range(6):
        gs = [g.double() for g in _grads_cpu(net, step)]
        for x, g in zip(net.parameters(), gs):
            x.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(list(net.parameters()), max_norm, foreach=True)
        opt.step()
        p, m, v, t, norm, coef, skipped = clipped_adam_step_ref(p, gs, m, v, t, kw["lr"], *kw["betas"], kw["eps"], kw["weight_decay"],
                                                                max_norm)
        assert not skipped and t == step + 1
        assert norm == pytest.approx(float(total), rel=1e-13)
        assert coef == coef_ref(norm, max_norm) and coef == pytest.approx(min(1.0, max_norm / (float(total) + 1e-6)), rel=1e-13)
        clipped.append(coef < 1.0)
        for a, b in zip(p, net.parameters()):
            assert torch.allclose(a, b.detach(), rtol=1e-12, atol=1e-14), step
    assert any(clipped) and not all(clipped), clipped
    # the guard: a non-finite gradient leaves everything as it was; without it the coefficient is NaN (torch.clamp lets NaN through)
    gs[0][0, 0, 0, 0] = float("nan")
    p2, m2, v2, t2, norm, coef, skipped = clipped_adam_step_ref(p, gs, m, v, t, kw["lr"], *kw["betas"], kw["eps"], 0.0, max_norm, True)
    assert skipped and t2 == t and all(torch.equal(a, b) for a, b in zip(p2 + m2 + v2, p + m + v))
    assert coef_ref(float("nan"), max_norm) != coef_ref(float("nan"), max_norm) and coef_ref(float("inf"), max_norm) == 0.0
    assert coef_ref(123.0, 0.0) == 1.0 and coef_ref(float("nan"), 0.0) == 1.0


# ---- host refusals: argument checks precede every launch, so these calls never reach a device ---------------------------------

FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced on the paths below
ERR_ARG = -1


def _sumsq(lib, g=FAKE, n=64, jobs=FAKE, table=((0, 16),), njobs=None, partials=FAKE, host_null=False):
    flat = [x for j in table for x in j]
    host = (ctypes.c_int64 * len(flat))(*flat)
    return lib.sst_grad_sumsq(g, n, jobs, None if host_null else ctypes.cast(host, ctypes.c_void_p), len(table) if njobs is None else njobs,
                              partials, None)


def _clip(lib, **kw):
    a = dict(p=FAKE, g=FAKE, m=FAKE, v=FAKE, ema=None, n=64, lr=FAKE, steps=FAKE, nsteps=1, partials=FAKE, npartials=1, max_norm=1.0,
             skip=1, rec=FAKE)
    a.update(kw)
    return lib.sst_adam_flat_clip(a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["lr"], a["steps"], a["nsteps"], 0.9, 0.999, 1e-4,
                                  0.0, 0.999, 1, a["partials"], a["npartials"], a["max_norm"], a["skip"], a["rec"], None)


def test_host_refusals_come_before_any_launch():
    from srganst import _abi
    lib = _abi.lib()

    def refused(rc, word):
        msg = lib.sst_last_error()
        assert rc == ERR_ARG and word in msg, (rc, msg)
        lib.sst_clear_error()

    for k in ("g", "jobs", "partials"):
        refused(_sumsq(lib, **{k: None}), b"null pointer")
    refused(_sumsq(lib, host_null=True), b"null pointer")
    refused(_sumsq(lib, n=62), b"multiple of 4")
    refused(_sumsq(lib, n=0), b"multiple of 4")
    refused(_sumsq(lib, njobs=0), b"njobs")
    refused(_sumsq(lib, g=FAKE + 4), b"16-byte aligned")
    refused(_sumsq(lib, table=((0, 16), (48, 17))), b"job 1 (start 48, count 17)")        # one element past n = 64
    refused(_sumsq(lib, table=((64, 1),)), b"job 0")
    refused(_sumsq(lib, table=((-1, 4),)), b"job 0")
    refused(_sumsq(lib, table=((0, 0),)), b"job 0")
    refused(_sumsq(lib, table=((8, 2 ** 62),)), b"job 0")                                # no overflow in start + count
    for k in ("p", "g", "m", "v", "lr", "steps", "partials", "rec"):
        refused(_clip(lib, **{k: None}), b"null pointer")
    refused(_clip(lib, n=66), b"multiple of 4")
    refused(_clip(lib, npartials=0), b"bad argument")
    refused(_clip(lib, max_norm=-1.0), b"max_norm")
    refused(_clip(lib, max_norm=float("nan")), b"max_norm")


def test_python_surface_refuses_bad_settings():
    from srganst.optim import FlatAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdam(_Net(), lr=1e-3, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdam(_Net(), lr=1e-3, max_grad_norm=float("nan"))
    off = FlatAdam(_Net(), lr=1e-3)
    assert not off.clip_on and off.grad_record is None and off.grad_stats() is None and off.clip_counters() is None


def test_config_keys_exist_and_default_to_off():
    from srganst.config import Config
    s = Config().SOLVER
    assert s.G_GRAD_CLIP == 0.0 and s.D_GRAD_CLIP == 0.0 and s.SKIP_NONFINITE is False
    from srganst.engine import _clip_knobs
    cfg = Config()
    assert _clip_knobs(cfg, "G") == (0.0, False) and _clip_knobs(cfg, "D") == (0.0, False)
    cfg.SOLVER.G_GRAD_CLIP, cfg.SOLVER.SKIP_NONFINITE = 5.0, True
    assert _clip_knobs(cfg, "G") == (5.0, True) and _clip_knobs(cfg, "D") == (0.0, True)


def test_training_state_carries_the_counters_only_when_the_feature_is_on(tmp_path):
    from srganst import checkpoint
    cfg = _ckpt_cfg()
    run = _ckpt_run(cfg, steps=1)
    off, on = str(tmp_path / "off.pth"), str(tmp_path / "on.pth")
    _ckpt_save(off, cfg, run)
    _ckpt_save(str(tmp_path / "none.pth"), cfg, run, clip=None)
    for f in (off, str(tmp_path / "none.pth")):
        assert "clip" not in checkpoint.load_training_state(f, "cpu", config=cfg, world_size=1)
    clip = {"G": {"n_skipped": 2, "n_clipped": 7, "n_steps_seen": 15}, "D": {"n_skipped": 1, "n_clipped": 0, "n_steps_seen": 8}}
    _ckpt_save(on, cfg, run, clip=clip)
    st = checkpoint.load_training_state(on, "cpu", config=cfg, world_size=1)            # weights_only loading
    assert st["clip"] == clip
    assert set(st) - {"clip"} == set(checkpoint.load_training_state(off, "cpu", config=cfg, world_size=1))
    assert st["format_version"] == checkpoint.FORMAT_VERSION == 1 and "clip" not in str(checkpoint.FINGERPRINT_FIELDS)
    # into an optimizer and back: a FlatAdam on the CPU keeps the record (the kernels are not involved)
    from srganst.optim import FlatAdam
    opt = FlatAdam(_Net(), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    assert opt.clip_counters() == {"n_skipped": 0, "n_clipped": 0, "n_steps_seen": 0}
    opt.load_clip_counters(None)                                                         # a file without the entry
    assert opt.clip_counters() == {"n_skipped": 0, "n_clipped": 0, "n_steps_seen": 0}
    opt.load_clip_counters(st["clip"]["G"])
    assert opt.clip_counters() == clip["G"]
    assert opt.grad_stats()["norm"] == 0.0 and set(opt.state_dict()) == {"state", "param_groups"}
