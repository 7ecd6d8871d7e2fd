"""GPU: global gradient-norm clipping and the non-finite step guard of the flat Adam (csrc/optim.hip: sst_grad_sumsq /
sst_adam_flat_clip) - the kernels through ops, optim.FlatAdam, the step engines and the drivers' resume.

Yardsticks: the fp64 restatement in tests/clip_refs.py for the norm and the coefficient; ops.adam_flat / ops.adam_flat_ema, bit
for bit, for the update (on g when coef == 1, on the fp32 product g * coef otherwise); torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam for FlatAdam's trajectory; and bitwise equality between eager and hipGraph replay, feature off and "on but
never active", DP schedule and single process, resumed and uninterrupted run."""
import math

import pytest
import torch

from clip_refs import coef_ref, norm_ref
from ema_refs import equal_tree, slot_mask, ulp_distance
from test_optim_gpu import _Net, _grads

pytestmark = pytest.mark.gpu

ADAM = (0.9, 0.999, 1e-4)          # betas, eps of the project's optimizers
REC = {"norm": 0, "coef": 1, "skipped_now": 2, "n_skipped": 3, "n_clipped": 4, "n_steps_seen": 5}


def _layout(name):
    """(offsets, numels, total, jobs).  one_slot: 16 floats.  net: the padded slots of test_optim_gpu._Net (1- and 3-element
    parameters).  chunk_plus_one: a slot whose second job has one element.  second_trip: 514 jobs - the finalising workgroup's
    256 threads loop over the partials three times - and the smallest size at which the update's grid-stride loop takes a second
    trip (tests/test_ema_gpu.py).  unaligned: a hand-made table whose jobs start off the 16-byte grid (scalar head, then float4s,
    then a scalar tail) with live words on both sides of every job."""
    from srganst import ops
    from srganst.optim import NORM_CHUNK, norm_jobs
    if name == "unaligned":
        offs, numels, total = [3, 70, 1030], [9, 953, 2], 1088
        return offs, numels, total, norm_jobs(offs, numels, 700)
    if name == "net":
        params = list(_Net().parameters())
        offs, total = ops.flat_layout(params)
        numels = [p.numel() for p in params]
    else:
        n = {"one_slot": 16, "chunk_plus_one": NORM_CHUNK + 1, "second_trip": 4 * (4096 * 256) + 64}[name]
        numels = [n] if name == "one_slot" else [3, n]                # a 3-element slot in front: 13 pad words before the big one
        offs, total = ops.flat_layout([torch.empty(k) for k in numels])
    return offs, numels, total, norm_jobs(offs, numels)


LAYOUTS = ["one_slot", "net", "chunk_plus_one", "second_trip", "unaligned"]


class _Case:
    """Flat buffers of one layout plus everything sst_grad_sumsq / sst_adam_flat_clip need."""

    def __init__(self, name, seed=0, grad_scale=1.0):
        from srganst import ops
        self.offs, self.numels, self.n, jobs = _layout(name)
        self.mask = slot_mask(self.offs, self.numels, self.n, "cuda")
        self.jobs = ops.NormJobs(jobs, torch.device("cuda"))
        gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
        rnd = lambda scale=1.0: torch.randn(self.n, device="cuda", generator=gen) * scale
        self.p0, self.g, self.m0, self.v0, self.e0 = rnd(), rnd(grad_scale), rnd(0.1), rnd(0.1).square(), rnd()
        self.lr = torch.tensor(1e-2, device="cuda")
        self.partials = torch.zeros(self.jobs.njobs, device="cuda", dtype=torch.float64)
        self.record = torch.zeros(6, device="cuda", dtype=torch.float64)

    def state(self, t):
        return self.p0.clone(), self.m0.clone(), self.v0.clone(), self.e0.clone(), torch.full((3,), float(t - 1), device="cuda")

    def clip_step(self, p, m, v, ema, steps, wd, max_norm, skip, g=None):
        from srganst import ops
        g = self.g if g is None else g
        ops.grad_sumsq(g, self.jobs, self.partials)
        ops.adam_flat_clip(p, g, m, v, ema, self.lr, steps, *ADAM, wd, 0.999, True, self.partials, self.jobs.njobs, max_norm, skip,
                           self.record)
        return self.record.clone()


@pytest.mark.parametrize("name", LAYOUTS)
def test_norm_against_fp64_reference_ignores_pads_and_is_reproducible(name):
    """|norm - ref| <= n * 2^-52 * ref: squares of fp32 values are exact in double, each side's sum of n positive terms is within
    (n - 1) * 2^-53 relative whatever its order, and the square root halves a relative error."""
    c = _Case(name)
    n_valid = sum(c.numels)
    if name == "second_trip":
        assert c.jobs.njobs > 2 * 256
    p, m, v, _, steps = c.state(1)
    rec = c.clip_step(p, m, v, None, steps, 0.0, 0.0, True)
    ref = norm_ref(c.g, c.offs, c.numels)
    norm = float(rec[REC["norm"]])
    err, bound = abs(norm - ref), n_valid * 2.0 ** -52 * ref
    print(f"{name}: n={n_valid} jobs={c.jobs.njobs} norm={norm!r} ref={ref!r} |diff|={err:.3e} bound={bound:.3e}")
    assert err <= bound
    assert rec.tolist()[1:] == [1.0, 0.0, 0.0, 0.0, 1.0]
    parts = c.partials.clone()
    assert math.sqrt(float(parts.sum())) == pytest.approx(norm, rel=1e-14)
    # pad words are never read: NaN or 1e30 in every one of them changes no bit of the partials, the norm or the decision
    assert (int((~c.mask).sum()) > 0) == (name != "one_slot")
    for fill in (float("nan"), 1e30):
        g = c.g.clone()
        g[~c.mask] = fill
        p, m, v, _, steps = c.state(1)
        rec2 = c.clip_step(p, m, v, None, steps, 0.0, 0.0, True, g=g)
        assert torch.equal(c.partials, parts), fill
        assert torch.equal(rec2[:3], rec[:3]) and float(rec2[REC["skipped_now"]]) == 0.0, fill
        assert float(steps[0]) == 1.0
    # two launches: the same bits
    p, m, v, _, steps = c.state(1)
    rec3 = c.clip_step(p, m, v, None, steps, 0.0, 0.0, True)
    assert torch.equal(c.partials, parts) and torch.equal(rec3[:3], rec[:3])
    assert float(rec3[REC["n_steps_seen"]]) == 4.0 and float(rec3[REC["n_skipped"]]) == 0.0


@pytest.mark.parametrize("name", ["net", "second_trip"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_update_with_coef_one_is_todays_update_bit_for_bit(name, wd):
    from srganst import ops
    c = _Case(name, seed=1)
    for t in (1, 10 ** 4):
        p, m, v, _, steps = c.state(t)
        ops.adam_flat(p, c.g, m, v, c.lr, steps, *ADAM, wd)
        pe, me, ve, ee, steps_e = c.state(t)
        ops.adam_flat_ema(pe, c.g, me, ve, ee, c.lr, steps_e, *ADAM, wd, 0.999, True)
        assert float(steps[0]) == t and not torch.equal(p, c.p0)
        for max_norm, skip in ((0.0, True), (1e30, False), (1e30, True)):
            for with_ema in (False, True):
                p2, m2, v2, e2, steps2 = c.state(t)
                rec = c.clip_step(p2, m2, v2, e2 if with_ema else None, steps2, wd, max_norm, skip)
                assert float(rec[REC["coef"]]) == 1.0 and float(rec[REC["skipped_now"]]) == 0.0
                assert torch.equal(steps2, steps), (t, max_norm, skip)
                assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v), (t, max_norm, skip, with_ema)
                assert torch.equal(e2, ee if with_ema else c.e0), (t, max_norm, skip)
    assert float(c.record[REC["n_clipped"]]) == 0.0 and float(c.record[REC["n_steps_seen"]]) == 12.0


@pytest.mark.parametrize("name", ["net", "second_trip", "unaligned"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_update_with_coef_below_one_is_the_update_on_the_scaled_gradient(name, wd):
    from srganst import ops
    c = _Case(name, seed=2)
    c.g[~c.mask] = float("nan")                                       # pads: neither in the norm nor in any parameter element
    ref = norm_ref(c.g, c.offs, c.numels)
    max_norm = 1.0
    assert ref > 2.0
    for t in (1, 10 ** 4):
        for with_ema in (False, True):
            p2, m2, v2, e2, steps2 = c.state(t)
            rec = c.clip_step(p2, m2, v2, e2 if with_ema else None, steps2, wd, max_norm, True)
            coef = rec[REC["coef"]].float()
            assert float(coef) == float(rec[REC["coef"]]) and 0.0 < float(coef) < 0.5           # an fp32 value, and it clips
            want = torch.tensor(coef_ref(ref, max_norm), dtype=torch.float64).float().cuda()
            ulps = ulp_distance(coef.reshape(1), want.reshape(1))
            print(f"{name} wd={wd} t={t}: coef={float(coef)!r} reference {float(want)!r} ({ulps} ulp)")
            assert ulps <= 1
            assert float(rec[REC["skipped_now"]]) == 0.0 and float(steps2[0]) == t
            scaled = c.g * coef                                      # torch's fp32 multiply
            p, m, v, e, steps = c.state(t)
            if with_ema:
                ops.adam_flat_ema(p, scaled, m, v, e, c.lr, steps, *ADAM, wd, 0.999, True)
            else:
                ops.adam_flat(p, scaled, m, v, c.lr, steps, *ADAM, wd)
            k = c.mask
            assert torch.equal(p2[k], p[k]) and torch.equal(m2[k], m[k]) and torch.equal(v2[k], v[k]), (t, with_ema)
            assert torch.equal(e2[k], e[k]) and bool(torch.isfinite(p2[k]).all())
            assert not torch.equal(m2[k], c.m0[k])
    assert float(c.record[REC["n_clipped"]]) == 4.0 == float(c.record[REC["n_steps_seen"]])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_gradient_is_skipped_with_the_guard_and_poisons_without(bad):
    from srganst import ops
    c = _Case("net", seed=3)
    t = 7
    where = c.offs[1]                                                 # the 1-element parameter: its pads follow right behind
    assert c.numels[1] == 1
    g_bad = c.g.clone()
    g_bad[where] = bad
    for max_norm in (0.0, 1.0):
        p, m, v, e, steps = c.state(t)
        before = [x.clone() for x in (p, m, v, e, steps)]
        c.record.zero_()
        rec = c.clip_step(p, m, v, e, steps, 0.01, max_norm, True, g=g_bad)
        for x, y in zip((p, m, v, e, steps), before):                 # nothing moved: weights, moments, average, step counters
            assert equal_tree(x, y)
        assert rec.tolist()[2:] == [1.0, 1.0, 0.0, 1.0] and not math.isfinite(float(rec[REC["norm"]]))
        rec = c.clip_step(p, m, v, e, steps, 0.01, max_norm, True, g=g_bad)
        assert rec.tolist()[2:] == [1.0, 2.0, 0.0, 2.0] and float(steps[0]) == t - 1
        # the next clean step takes the un-advanced step count: it is the update adam_flat_ema makes at t
        rec = c.clip_step(p, m, v, e, steps, 0.01, 1e30, True)
        pw, mw, vw, ew, sw = c.state(t)
        ops.adam_flat_ema(pw, c.g, mw, vw, ew, c.lr, sw, *ADAM, 0.01, 0.999, True)
        assert rec.tolist()[1:] == [1.0, 0.0, 2.0, 0.0, 3.0] and float(steps[0]) == t
        assert torch.equal(p, pw) and torch.equal(m, mw) and torch.equal(v, vw) and torch.equal(e, ew) and torch.equal(steps, sw)
    # guard off, clipping on: clip_grad_norm_'s arithmetic with error_if_nonfinite=False.  A NaN norm gives a NaN coefficient and
    # every parameter element becomes NaN; an infinite norm gives max_norm / inf = 0, i.e. the update on g * 0 (NaN where g is inf)
    p, m, v, e, steps = c.state(t)
    rec = c.clip_step(p, m, v, None, steps, 0.0, 1.0, False, g=g_bad)
    assert float(rec[REC["skipped_now"]]) == 0.0 and float(steps[0]) == t and float(rec[REC["n_skipped"]]) == 2.0
    coef = rec[REC["coef"]].float()
    if bad != bad:
        assert float(coef) != float(coef) and bool(torch.isnan(p[c.mask]).all())
    else:
        assert float(coef) == 0.0
    assert bool(torch.isnan(p[where]))
    pw, mw, vw, _, sw = c.state(t)
    ops.adam_flat(pw, g_bad * coef, mw, vw, c.lr, sw, *ADAM, 0.0)
    for x, y in ((p, pw), (m, mw), (v, vw)):
        assert torch.equal(torch.isnan(x[c.mask]), torch.isnan(y[c.mask]))
        assert torch.equal(torch.nan_to_num(x[c.mask]), torch.nan_to_num(y[c.mask]))


# ---- optim.FlatAdam ------------------------------------------------------------------------------------------------------------------

def _set_grads(net, names, gs, flat_path):
    from srganst import ops
    if flat_path:
        views = ops.flat_grads(net, names, list(net.parameters()))   # what the HIP backward passes hand to autograd
        for (n, p), g in zip(net.named_parameters(), gs):
            views[n].copy_(g)
            p.grad = views[n]
    else:
        for p, g in zip(net.parameters(), gs):
            p.grad = g.clone()


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("flat_path", [True, False])
def test_flat_adam_follows_torch_clip_and_adam(capturable, flat_path, monkeypatch):
    """Six steps of test_optim_gpu's gradients (norms about 12.6, 126, 1260 by turns; max_norm = 50 clips four of them) within the
    bound test_optim_gpu holds FlatAdam to; flat_path False = plain .grad tensors, i.e. torch's clip and torch's update."""
    from srganst._abi import HipPathError
    from srganst.optim import FlatAdam
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01)
    max_norm = 50.0
    ref_net, net = _Net().cuda(), _Net().cuda()
    ref = torch.optim.Adam(ref_net.parameters(), **kw)
    opt = FlatAdam(net, capturable=capturable, max_grad_norm=max_norm, skip_nonfinite=True, ema_decay=0.999, **kw)
    assert opt.clip_on and opt.grad_record.dtype == torch.float64 and opt.grad_stats()["n_steps_seen"] == 0
    names = [n for n, _ in net.named_parameters()]
    coefs = []
    for step in range(6):
        gs = _grads(net, step)
        for p, g in zip(ref_net.parameters(), gs):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref_net.parameters()), max_norm, foreach=True)
        ref.step()
        _set_grads(net, names, gs, flat_path)
        assert (opt._flat_grad() is not None) == flat_path
        opt.step()
        st = opt.grad_stats()
        assert st["norm"] == pytest.approx(float(total), rel=1e-5) and st["skipped_now"] == 0 and st["n_steps_seen"] == step + 1
        assert st["coef"] == pytest.approx(min(1.0, max_norm / (float(total) + 1e-6)), rel=1e-5)
        coefs.append(st["coef"])
        for (n, p), q in zip(net.named_parameters(), ref_net.parameters()):
            assert torch.allclose(p, q, rtol=2e-6, atol=1e-7), (step, n)
    assert [c < 1.0 for c in coefs] == [False, True, True] * 2 and opt.grad_stats()["n_clipped"] == 4
    # a non-finite gradient: nothing moves, on either path
    snap = [x.clone() for x in (opt._flat_p, opt._m, opt._v, opt._steps, opt.ema)]
    gs = _grads(net, 6)
    gs[2][1] = float("inf")
    _set_grads(net, names, gs, flat_path)
    opt.step()
    st = opt.grad_stats()
    assert (st["skipped_now"], st["n_skipped"], st["n_clipped"], st["n_steps_seen"]) == (1, 1, 4, 7)
    for x, y in zip((opt._flat_p, opt._m, opt._v, opt._steps, opt.ema), snap):
        assert torch.equal(x, y)
    assert opt.clip_counters() == {"n_skipped": 1, "n_clipped": 4, "n_steps_seen": 7}
    sd = opt.state_dict()                                             # torch's layout, nothing of ours in it
    assert set(sd) == {"state", "param_groups"} and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    if not flat_path:                                                 # the host decision of the stock path cannot be captured
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(HipPathError, match="cannot be captured"):
            opt.step()


# ---- engines -------------------------------------------------------------------------------------------------------------------------

def _cfg(g_clip, d_clip, guard, d_interval=2):
    from test_ema_gpu import _cfg as ema_cfg
    cfg = ema_cfg(0.999)
    cfg.SOLVER.D_UPDATE_INTERVAL = d_interval
    cfg.SOLVER.G_GRAD_CLIP, cfg.SOLVER.D_GRAD_CLIP, cfg.SOLVER.SKIP_NONFINITE = g_clip, d_clip, guard
    return cfg


def _opt_tensors(eng, kind):
    out = {}
    for net, opt in (("G", eng.opt if kind == "warmup" else eng.g_opt), ("D", None if kind == "warmup" else eng.d_opt)):
        if opt is None:
            continue
        for k, t in (("p", opt._flat_p), ("m", opt._m), ("v", opt._v), ("steps", opt._steps), ("ema", opt.ema), ("rec", opt.grad_record)):
            if t is not None:
                out[f"{net}.{k}"] = t.clone()
    return out


def _build(kind, cfg, use_graph, force_dp=False):
    from srganst.engine import TrainEngine, WarmupEngine
    from srganst.model import Discriminator, Generator
    torch.manual_seed(1)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    if kind == "warmup":
        return WarmupEngine(cfg, G, use_graph=use_graph, adam_capturable=True, force_dp=force_dp), G, D
    return TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True, force_dp=force_dp), G, D


def _batches(n, seed=2):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 96, 96, generator=gen).cuda(), torch.rand(4, 3, 24, 24, generator=gen).cuda()) for _ in range(n)]


def _run(kind, clips, use_graph, overlap_gd=True, force_dp=False, iters=6):
    cfg = _cfg(*clips)
    cfg.KERNEL.OVERLAP_GD = overlap_gd
    eng, G, D = _build(kind, cfg, use_graph, force_dp)
    for gt, lr in _batches(iters):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    assert eng.graph_active == use_graph
    out = _opt_tensors(eng, kind)
    out.update({"G.sd." + k: v.clone() for k, v in G.state_dict().items()})
    out.update({"loss." + k: v.clone() for k, v in eng.loss_values.items()})
    if kind == "train":
        out.update({"D.sd." + k: v.clone() for k, v in D.state_dict().items()})
    stats = eng.grad_stats()
    eng.close()
    return out, stats


@pytest.fixture(scope="module")
def half_norms():
    """Half the gradient norms a first eager iteration records, per engine kind: clipping then really happens."""
    out = {}
    for kind in ("warmup", "train"):
        eng, _, _ = _build(kind, _cfg(1e30, 1e30, True), False)
        eng.step(*_batches(1)[0])
        st = eng.grad_stats()
        eng.close()
        assert st["G"]["coef"] == 1.0 and st["G"]["norm"] > 0 and (kind == "warmup") == (st["D"] is None)
        out[kind] = (st["G"]["norm"] / 2, 0.0 if st["D"] is None else st["D"]["norm"] / 2)
    return out


def _same(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert equal_tree(a[k], b[k]), k


@pytest.mark.parametrize("kind,overlap_gd", [("warmup", True), ("train", True), ("train", False)])
def test_engine_graph_replay_equals_eager_with_clipping(kind, overlap_gd, half_norms):
    clips = (*half_norms[kind], True)
    eager, st_e = _run(kind, clips, False, overlap_gd)
    graph, st_g = _run(kind, clips, True, overlap_gd)
    _same(eager, graph)                                               # parameters, moments, average, record, BatchNorm buffers, losses
    assert st_e == st_g and st_g["G"]["n_steps_seen"] == 6 and st_g["G"]["n_clipped"] >= 1 and st_g["G"]["n_skipped"] == 0
    if kind == "train":
        assert st_g["D"]["n_steps_seen"] == 3 and st_g["D"]["n_clipped"] >= 1 and st_g["D"]["n_skipped"] == 0
    else:
        assert st_g["D"] is None


@pytest.mark.parametrize("kind", ["warmup", "train"])
def test_engine_with_a_bound_never_reached_equals_the_feature_off(kind):
    off, st_off = _run(kind, (0.0, 0.0, False), True)
    on, st_on = _run(kind, (1e30, 1e30, True), True)
    assert st_off == {"G": None, "D": None} and st_on["G"]["n_clipped"] == 0 and st_on["G"]["n_skipped"] == 0
    assert not any(k.endswith(".rec") for k in off)
    _same(off, {k: v for k, v in on.items() if not k.endswith(".rec")})


@pytest.mark.parametrize("kind", ["warmup", "train"])
def test_engine_dp_schedule_equals_single_process(kind, half_norms):
    """force_dp with one rank: the split graphs of the data-parallel schedules ([forward + backward] -> collective -> [optimizer]),
    the optimizer step - norm, decision, update - in a graph of its own behind the all-reduce's wait."""
    clips = (*half_norms[kind], True)
    single, st_s = _run(kind, clips, True)
    dp, st_d = _run(kind, clips, True, force_dp=True)
    _same(single, dp)
    assert st_s == st_d and st_d["G"]["n_clipped"] >= 1


def test_engine_skips_a_nan_batch_inside_the_captured_graph(half_norms):
    cfg = _cfg(*half_norms["train"], True, d_interval=1)
    eng, G, D = _build("train", cfg, True)
    batches = _batches(6, seed=5)
    for gt, lr in batches[:4]:
        eng.step(gt, lr)
    torch.cuda.synchronize()
    assert eng.graph_active
    snap = _opt_tensors(eng, "train")
    gt, lr = batches[4]
    gt = gt.clone()
    gt[1, 2, 40, 17] = float("nan")
    eng.step(gt, lr)
    torch.cuda.synchronize()
    st = eng.grad_stats()
    assert st["G"]["skipped_now"] == 1 and st["D"]["skipped_now"] == 1 and st["G"]["n_skipped"] == 1 and st["D"]["n_skipped"] == 1
    assert st["G"]["n_steps_seen"] == 5 and st["D"]["n_steps_seen"] == 5
    _same(snap, _opt_tensors(eng, "train"), skip=("G.rec", "D.rec"))   # flat parameters, moments, step counters, the average
    assert not bool(torch.isfinite(eng.d_loss).all())
    loss_values, d_loss = eng.step(*batches[5])
    torch.cuda.synchronize()
    assert eng.graph_active
    assert all(bool(torch.isfinite(v).all()) for v in loss_values.values()) and bool(torch.isfinite(d_loss).all())
    after, st = _opt_tensors(eng, "train"), eng.grad_stats()
    assert st["G"]["skipped_now"] == 0 and st["D"]["skipped_now"] == 0 and st["G"]["n_skipped"] == 1 and st["D"]["n_skipped"] == 1
    for net in ("G", "D"):
        assert not torch.equal(after[net + ".p"], snap[net + ".p"]) and bool(torch.isfinite(after[net + ".p"]).all())
        assert torch.equal(after[net + ".steps"], snap[net + ".steps"] + 1)
    assert bool(torch.isfinite(after["G.ema"]).all()) and not torch.equal(after["G.ema"], snap["G.ema"])
    eng.close()


# ---- drivers: the counters travel with the training state ---------------------------------------------------------------------------

def test_resumed_run_with_clipping_equals_uninterrupted_run(tmp_path, half_norms):
    from test_resume_gpu import _cfg as resume_cfg, _drive, _in_dir, _load

    def cfg(name, **exp):
        c = resume_cfg(tmp_path, name, "train", **exp)
        c.SOLVER.G_GRAD_CLIP, c.SOLVER.D_GRAD_CLIP = half_norms["train"]
        c.SOLVER.SKIP_NONFINITE = True
        return c
    with _in_dir(tmp_path):
        logged = _drive("train", cfg("clip_A", N_EPOCHS=2))
        _drive("train", cfg("clip_B", N_EPOCHS=1))
        first = _load("clip_B", "state_last.pth")
        assert first["epoch"] == 1 and first["clip"]["G"]["n_steps_seen"] == 5 and first["clip"]["D"]["n_steps_seen"] == 3
        _drive("train", cfg("clip_B", N_EPOCHS=2, RESUME="auto"))
        for f in ("g_last.pth", "d_last.pth", "g_ema_last.pth"):
            assert equal_tree(_load("clip_A", f), _load("clip_B", f)), f
        sa, sb = _load("clip_A", "state_last.pth"), _load("clip_B", "state_last.pth")
        assert sa["clip"] == sb["clip"] and set(sa["clip"]) == {"G", "D"}
        assert sa["clip"]["G"]["n_steps_seen"] == 10 and sa["clip"]["D"]["n_steps_seen"] == 6
        assert sa["clip"]["G"]["n_clipped"] > first["clip"]["G"]["n_clipped"] > 0 and sa["clip"]["G"]["n_skipped"] == 0
        assert equal_tree(sa["g_opt"], sb["g_opt"]) and equal_tree(sa["d_opt"], sb["d_opt"]) and equal_tree(sa["rng"], sb["rng"])
        tags = {t for t, _ in logged}
        assert {"Train/G_GradNorm", "Train/D_GradNorm", "Train/G_ClipCoef", "Train/D_ClipCoef", "Train/G_Skipped", "Train/D_Skipped"} <= tags
