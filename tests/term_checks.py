"""What the GPU tests of the criteria behind the term protocol (srganst.loss._Term: SSIMLoss, FocalFrequencyLoss, BackProjectionLoss,
and the general route of StructureTensorLoss) ask of each of them alike - determinism, graph capture, no_grad, the engines and the
refusals.  A plain helper module: the test functions, their parametrisations and what is particular to a criterion (its cases,
its restatement, its refused pairs) stay in tests/test_*_gpu.py, which call in here."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_fp64_truth, oracle_grads, rel_err


def ws_ptrs(crit, keys):
    return tuple(crit._ws[k].data_ptr() for k in keys)


def two_calls_give_equal_bits(calls):
    """calls: functions of nothing -> a tuple of tensors, each from a fresh launch."""
    for call in calls:
        a, b = call(), call()
        assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def fwd_bwd(crit, xs, gs):
    loss = crit(xs, gs)
    (gx,) = torch.autograd.grad(loss, xs)
    return loss, gx


def graph_replay_matches_eager(make, inputs, pointers, run=fwd_bwd, order=(1, 2, 0)):
    """run(make(), xs, gs) -> tensors (forward + backward), captured after one warm-up call on a side stream (which allocates the
    workspace) and replayed on the three `inputs` copied into the static tensors: every output's bits equal the eager calls' each
    time, so the ticket counter re-arms inside the graph; pointers(made, xs) -> the addresses the capture must not move.
    -> what make() gave the captured calls."""
    eager = []
    for x, gt in inputs:
        out = run(make(), x.cuda().requires_grad_(True), gt.cuda())
        eager.append(tuple(t.detach().clone() for t in out))
    torch.cuda.synchronize()
    assert not torch.equal(eager[1][0], eager[2][0])

    made = make()
    xs = inputs[0][0].cuda().requires_grad_(True)
    gs = inputs[0][1].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(made, xs, gs)                                                # warm-up: allocates the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ptrs = pointers(made, xs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(made, xs, gs)
    assert pointers(made, xs) == ptrs                                    # nothing of the workspace was re-allocated in the capture
    for k in order:
        with torch.no_grad():
            xs.copy_(inputs[k][0])
            gs.copy_(inputs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        for i, (got, want) in enumerate(zip(out, eager[k])):
            assert torch.equal(got, want), (k, i, got, want)
    del graph
    return made


def no_grad_allocates_and_writes_nothing_saved(monkeypatch, crit, x, gt, saved_bytes, kernel, raw_loss):
    """Under no_grad, and where sr does not require a gradient: the same loss bits, what the backward would read (keep[3] of the
    forward's trace entry) is neither allocated nor written, and raw_loss(xd, gd) - the entry through the ABI with a null pointer in
    its place - gives the same bits again.  saved_bytes: the size of what is not allocated."""
    from srganst import ops
    xd, gd = x.cuda(), gt.cuda()
    xg = xd.clone().requires_grad_(True)
    with_grad = crit(xg, gd)                                            # also allocates the workspace
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = crit(xg, gd)
    plain = crit(xd, gd)                                                # grad mode on, sr does not require grad
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.equal(quiet, with_grad) and torch.equal(plain, with_grad)
    assert not quiet.requires_grad and not plain.requires_grad
    assert list(ops.TRACE_HBM) == [kernel]                              # two forward entries, no backward
    calls = ops.TRACE_HBM[kernel]
    assert len(calls) == 2 and all(keep[3] is None for _, _, keep in calls)        # keep = (x, gt, loss, saved, ws, ...)
    assert all(nbytes == 2.0 * x.numel() * 4 for _, nbytes, _ in calls)            # algorithmic bytes: sr + gt
    assert peak < saved_bytes, (peak, saved_bytes)                      # only the two 0-dim results were allocated
    assert torch.equal(raw_loss(xd, gd), with_grad.detach())


def _reduced_cfg(rcb=2):
    from srganst.config import Config
    cfg = Config()
    cfg.MODEL.G_N_RCB = rcb
    return cfg


def warmup_engine_step_vs_oracle(make, name, weight, ref):
    """One eager warm-up step with Pixel (MSE) + weight * the criterion, B = 4, 96 -> 24 px, two residual blocks: SR, the logged
    values and every parameter gradient against the CPU oracle of mse + weight * ref(sr, gt) (fp64-truth rule)."""
    from oracle import model as om
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss
    from srganst.model import Generator
    cfg = _reduced_cfg()
    torch.manual_seed(41)
    G = Generator(cfg)
    sd0 = {k: v.clone() for k, v in G.state_dict().items()}
    gen = torch.Generator().manual_seed(42)
    gt = torch.rand(4, 3, 96, 96, generator=gen)
    lr = torch.rand(4, 3, 24, 24, generator=gen)

    def fl(sdx, lr_, gt_):
        sr_ = om.generator_forward(sdx, lr_, True, {})
        mse, term = F.mse_loss(sr_, gt_), ref(sr_, gt_)
        return mse + weight * term, sr_, mse, term
    ins = ((lr, False), (gt, False))
    _, g32, _, (sr_ref, mse32, t32) = oracle_grads(fl, sd0, torch.float32, ins)
    _, g64, _, (_, mse64, t64) = oracle_grads(fl, sd0, torch.float64, ins)
    G.cuda().train()
    eng = WarmupEngine(cfg, G, {"Pixel": MSELoss(), name: make()}, {"Pixel": 1.0, name: weight}, use_graph=False)
    vals = eng.step(gt.cuda(), lr.cuda())
    assert rel_err(eng.sr.cpu(), sr_ref) < 1e-3
    assert list(vals) == ["Pixel", name]
    assert abs(vals["Pixel"].item() - mse64.item()) <= 1e-3 * mse64.item()
    e = abs(vals[name].item() - weight * t64.item())
    print(f"[warm-up] {name} term {vals[name].item():.7e} oracle fp64 {weight * t64.item():.7e} (fp32 {weight * t32.item():.7e})")
    assert e <= 1e-3 * weight * t64.item()                              # SR itself carries 1e-3: the term is not held tighter
    report = []
    for n, p in G.named_parameters():
        assert_fp64_truth(n, p.grad.cpu(), g32[n], g64[n], report)
    print(f"[warm-up] worst parameter-gradient error {max(r[1] for r in report):.3e}")
    eng.close()


def warmup_engine_graph_equals_eager(make, name, weight):
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss
    from srganst.model import Generator

    def run(use_graph):
        cfg = _reduced_cfg()
        torch.manual_seed(43)
        G = Generator(cfg).cuda().train()
        eng = WarmupEngine(cfg, G, {"Pixel": MSELoss(), name: make()}, {"Pixel": 1.0, name: weight}, use_graph=use_graph,
                           adam_capturable=True)
        gen = torch.Generator().manual_seed(44)
        logged = []
        for _ in range(3):
            gt = torch.rand(4, 3, 96, 96, generator=gen).cuda()
            lr = torch.rand(4, 3, 24, 24, generator=gen).cuda()
            logged.append({k: v.item() for k, v in eng.step(gt, lr).items()})
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph
        sd = {k: v.clone() for k, v in G.state_dict().items()}
        eng.close()
        return sd, logged

    s1, l1 = run(False)
    s2, l2 = run(True)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert l1 == l2 and all(set(v) == {"Pixel", name} for v in l1)


def train_engine_graph_equals_eager(make, name, weight):
    """Adversarial + Pixel + the criterion in a reduced TrainEngine: the criterion sits in the two-branch graph beside the
    discriminator; replayed and eager steps leave the same bits (the pattern of tests/test_discriminator_gpu.py)."""
    from srganst.config import Config
    from srganst.engine import TrainEngine
    from srganst.loss import MSELoss
    from srganst.model import Discriminator, Generator

    def run(use_graph):
        cfg = Config()
        cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
        torch.manual_seed(1)
        D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
        cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
        cfg.add_g_criterion(name, make(), weight)
        cfg.SOLVER.D_UPDATE_INTERVAL = 1
        eng = TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True)
        gen = torch.Generator().manual_seed(2)
        for _ in range(4):
            gt = torch.rand(4, 3, 96, 96, generator=gen).cuda()
            lr = torch.rand(4, 3, 24, 24, generator=gen).cuda()
            eng.step(gt, lr)
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph
        return G.state_dict(), D.state_dict(), {k: v.item() for k, v in eng.loss_values.items()}

    g1, d1, l1 = run(False)
    g2, d2, l2 = run(True)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in d1:
        assert torch.equal(d1[k], d2[k]), k
    assert l1 == l2 and set(l1) == {"Adversarial", "Pixel", name}


def refusals_launch_nothing(monkeypatch, refused, accepted, kernel):
    """refused: (criterion, a, b) or (criterion, a, b, a fragment of the message) - each raises HipPathError, and afterwards nothing
    was launched and no criterion holds a workspace (or tables).  accepted: (criterion, a, b) - the smallest sizes, as
    non-contiguous views: each gives a finite loss from one launch of `kernel`."""
    from srganst import ops
    from srganst._abi import HipPathError
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    for crit, a, b, *fragment in refused:
        with pytest.raises(HipPathError) as info:
            crit(a, b)
        assert all(f in str(info.value) for f in fragment), (fragment, str(info.value))
    assert ops.TRACE_HBM == {}
    assert all(crit._ws == {} and getattr(crit, "_tab", {}) == {} for crit, *_ in refused)
    for crit, a, b in accepted:
        assert torch.isfinite(crit(a, b))
    assert list(ops.TRACE_HBM) == [kernel] and len(ops.TRACE_HBM[kernel]) == len(accepted)
