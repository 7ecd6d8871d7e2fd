"""GPU: the generator weight average kept by the flat Adam kernel (csrc/optim.hip: sst_adam_flat_ema / sst_ema_flat) - the kernels
through ops, optim.FlatAdam, and the step engines' shadow generator (engine.g_ema).

Yardstick: the fp64 restatement in tests/ema_refs.py.  Both sides are a double result rounded once to fp32 and can differ only by
FMA contraction in double: at most ONE fp32 ulp, compared through the int32 view, pad words excluded.  Adam's own outputs must be
bit-identical to sst_adam_flat's."""
import pytest
import torch

from ema_refs import ema_ref, slot_mask, ulp_distance
from test_optim_gpu import _Net, _grads

pytestmark = pytest.mark.gpu

DECAY = 0.999


def _net_layout():
    from srganst import ops
    params = list(_Net().parameters())
    offs, total = ops.flat_layout(params)
    return offs, [p.numel() for p in params], total


# 16: one slot.  "net": the padded slots of test_optim_gpu._Net (a 1-element and a 3-element parameter).  The grid is capped at 4096
# workgroups of 256 float4 lanes, so 4 * 4096 * 256 + 64 floats is the smallest size whose grid-stride loop takes a second, partial trip.
SIZES = {"one_slot": 16, "net": None, "second_trip": 4 * (4096 * 256) + 64}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_kernel_against_adam_flat_and_fp64_rule(size, wd):
    from srganst import ops
    if size == "net":
        offs, numels, n = _net_layout()
        assert 1 in numels and 3 in numels and n > sum(numels)
    else:
        n = SIZES[size]
        offs, numels = [0], [n]
    mask = slot_mask(offs, numels, n, "cuda")
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + int(wd * 100))
    rnd = lambda scale=1.0: torch.randn(n, device="cuda", generator=g) * scale
    p0, grad, m0, v0, e0 = rnd(), rnd(), rnd(0.1), rnd(0.1).square(), rnd()
    lr = torch.tensor(1e-2, device="cuda")
    for t in (1, 2, 9, 10 ** 4):
        for warm in (True, False):
            steps = torch.full((3,), float(t - 1), device="cuda")
            p, m, v = p0.clone(), m0.clone(), v0.clone()
            ops.adam_flat(p, grad, m, v, lr, steps, 0.9, 0.999, 1e-4, wd)
            assert float(steps[0]) == t
            steps2 = torch.full((3,), float(t - 1), device="cuda")
            p2, m2, v2, e2 = p0.clone(), m0.clone(), v0.clone(), e0.clone()
            ops.adam_flat_ema(p2, grad, m2, v2, e2, lr, steps2, 0.9, 0.999, 1e-4, wd, DECAY, warm)
            assert torch.equal(steps2, steps)
            assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v), (t, warm)
            want = ema_ref(e0, p, t, DECAY, warm)
            ulps = ulp_distance(e2[mask], want[mask])
            print(f"n={n} wd={wd} t={t} warmup={warm}: max ulp distance {ulps}")
            assert ulps <= 1, (t, warm, ulps)
            assert not torch.equal(e2, e0)
            # the update alone (the stock-torch fallback's path): same rule, same bits, counters untouched
            e3 = e0.clone()
            ops.ema_flat(e3, p, steps, DECAY, warm)
            assert torch.equal(e3, e2), (t, warm)
            assert float(steps[0]) == t


def _set_flat_grads(net, names, gs):
    from srganst import ops
    views = ops.flat_grads(net, names, list(net.parameters()))         # what the HIP backward passes hand to autograd
    for (n, p), g in zip(net.named_parameters(), gs):
        views[n].copy_(g)
        p.grad = views[n]


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("flat_path", [True, False])
def test_flat_adam_keeps_the_average(capturable, flat_path):
    """Six steps; flat_path False = plain .grad tensors, i.e. torch's own update followed by sst_ema_flat."""
    from srganst.optim import FlatAdam
    net, base = _Net().cuda(), _Net().cuda()
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01, capturable=capturable)
    opt = FlatAdam(net, ema_decay=DECAY, **kw)
    ref = FlatAdam(base, ema_decay=0.0, **kw)
    assert ref.ema is None and opt.ema is not None and opt.ema.data_ptr() != opt._flat_p.data_ptr()
    assert torch.equal(opt.ema, opt._flat_p)                           # filled at construction
    names = [n for n, _ in net.named_parameters()]
    mask = slot_mask(opt._offs, [p.numel() for p in opt._params], opt._flat_p.numel(), "cuda")
    for step in range(6):
        gs = _grads(net, step)
        for o, m in ((opt, net), (ref, base)):
            if flat_path:
                _set_flat_grads(m, names, gs)
            else:
                for p, g in zip(m.parameters(), gs):
                    p.grad = g.clone()
            assert (o._flat_grad() is not None) == flat_path
        prev = opt.ema.clone()
        opt.step()
        ref.step()
        assert float(opt._steps[0]) == step + 1
        for p, q in zip(net.parameters(), base.parameters()):
            assert torch.equal(p, q), step                             # the average does not perturb the update
        want = ema_ref(prev, opt._flat_p, step + 1, DECAY, True)
        ulps = ulp_distance(opt.ema[mask], want[mask])
        print(f"capturable={capturable} flat_path={flat_path} step {step + 1}: max ulp distance {ulps}")
        assert ulps <= 1, (step, ulps)
    assert not torch.equal(opt.ema[mask], opt._flat_p[mask])
    # state_dict stays torch.optim.Adam's layout: the average is not in it
    stock = torch.optim.Adam(_Net().cuda().parameters(), fused=True, **kw)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == len(names)
    assert set(sd["param_groups"][0]) == set(stock.state_dict()["param_groups"][0])
    opt.reset_ema()
    assert torch.equal(opt.ema, opt._flat_p)


# ---- engines -----------------------------------------------------------------------------------------------------------------------

def _cfg(ema_decay):
    from srganst.config import Config
    from srganst.loss import MSELoss, StructureTensorLoss
    cfg = Config()
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
    cfg.DATA.BATCH_SIZE = 4
    cfg.SOLVER.D_UPDATE_INTERVAL = 2
    cfg.SOLVER.G_EMA_DECAY = ema_decay
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
    return cfg


def _run_engine(kind, ema_decay, use_graph, overlap_gd=True):
    """Six steps of the driver test's size; returns every tensor the comparison needs (cloned) and, with the average on, the
    eval-mode outputs of the shadow and of G on one LR batch."""
    from srganst import ops
    from srganst.engine import TrainEngine, WarmupEngine
    from srganst.model import Discriminator, Generator
    cfg = _cfg(ema_decay)
    cfg.KERNEL.OVERLAP_GD = overlap_gd
    assert not ops.conv_acc_supported(4, 24, 24, 16, 16)             # no fp64-atomic statistics here: every reduction is fixed-order
    torch.manual_seed(1)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    cpu_rng = torch.get_rng_state()
    if kind == "warmup":
        eng = WarmupEngine(cfg, G, use_graph=use_graph, adam_capturable=True)
    else:
        eng = TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True)
    assert torch.equal(torch.get_rng_state(), cpu_rng)                # building the shadow draws nothing from the global stream
    assert (eng.g_ema is None) == (ema_decay == 0)
    gen = torch.Generator().manual_seed(2)
    for _ in range(6):
        eng.step(torch.rand(4, 3, 96, 96, generator=gen).cuda(), torch.rand(4, 3, 24, 24, generator=gen).cuda())
    torch.cuda.synchronize()
    assert eng.graph_active == use_graph
    out = {"G." + k: v.clone() for k, v in G.state_dict().items()}
    out.update({"loss." + k: v.clone() for k, v in eng.loss_values.items()})
    if kind == "train":
        out.update({"D." + k: v.clone() for k, v in D.state_dict().items()})
        out["d_loss"] = eng.d_loss.clone()
    ema = None
    if eng.g_ema is not None:
        opt = eng.opt if kind == "warmup" else eng.g_opt
        shadow = eng.g_ema
        assert not shadow.training
        flat = opt.ema                                                # ONE buffer: the shadow's parameters are views of it
        assert all(p.data_ptr() == flat.data_ptr() + 4 * o for p, o in zip(shadow.parameters(), opt._offs))
        bn = [k for k, _ in G.named_buffers()]
        assert bn and not all(torch.equal(dict(shadow.named_buffers())[k], dict(G.named_buffers())[k]) for k in bn)
        eng.sync_ema_buffers()
        assert all(torch.equal(dict(shadow.named_buffers())[k], dict(G.named_buffers())[k]) for k in bn)
        lr = torch.rand(2, 3, 24, 24, generator=gen).cuda()
        with torch.no_grad():
            y_ema = shadow(lr)
            y_g = G.eval()(lr)
        assert not shadow.training and y_ema.shape == (2, 3, 96, 96) and bool(torch.isfinite(y_ema).all())
        assert not torch.equal(y_ema, y_g)                            # the average is not the last iterate
        ema = {k: v.clone() for k, v in shadow.state_dict().items()}
    eng.close()
    assert eng.g_ema is None
    return out, ema


@pytest.mark.parametrize("kind,overlap_gd", [("warmup", True), ("train", True), ("train", False)])
def test_engine_average_rides_in_the_graph_and_leaves_training_alone(kind, overlap_gd):
    eager, ema_eager = _run_engine(kind, DECAY, False, overlap_gd)
    graph, ema_graph = _run_engine(kind, DECAY, True, overlap_gd)
    for k in ema_eager:
        assert torch.equal(ema_eager[k], ema_graph[k]), k             # replayed from the hipGraph = eager, bit for bit
    off, none = _run_engine(kind, 0.0, True, overlap_gd)
    assert none is None
    assert set(off) == set(graph) == set(eager)
    for k in off:                                                     # parameters, BatchNorm buffers, loss values
        assert torch.equal(off[k], graph[k]) and torch.equal(off[k], eager[k]), k
    # the shadow holds an average: away from G's weights, between the initial and the last iterate's scale
    assert any(not torch.equal(ema_graph[k], graph["G." + k]) for k in ema_graph if k.endswith("weight"))
