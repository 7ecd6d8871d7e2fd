"""srganst._state on the CPU: the per-module HipState stays invisible to torch's module API, its scoped fields restore
themselves however their body ends, and the two identity checks built on it (dist.module_flat_grad, KeptPass.is_pass_over)."""
import pytest
import torch

from srganst._state import KeptPass, state


def _small(kind):
    from srganst.config import Config
    from srganst.model import Discriminator, Generator
    cfg = Config()
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 8, 1, 8
    torch.manual_seed(0)
    return Discriminator(cfg) if kind == "D" else Generator(cfg)


def _kept(x, pd):
    return KeptPass(x.data_ptr(), tuple(x.shape), None, None, pd, None)


@pytest.mark.parametrize("kind", ["D", "G"])
def test_state_stays_out_of_the_module_api(kind):
    from srganst import disc_graph, ops
    m = _small(kind)

    def listing():
        return (list(m.state_dict().keys()), [n for n, _ in m.named_parameters()], [n for n, _ in m.named_buffers()],
                [n for n, _ in m.named_modules()])
    before = listing()
    values = {k: v.clone() for k, v in m.state_dict().items()}
    st = state(m)
    assert state(m) is st
    # filled by the code that fills it in a run (the two that need no device) ...
    ops.flatten_bn_counters(m)
    ops.flatten_params(m)
    assert st.nbt_flat is not None and st.flat_params is not None
    # ... and by hand: every other field
    st.cache["pack"] = torch.zeros(3)
    st.flat_ring = {"total": 4, "device": torch.device("cpu"), "next": 0, "bufs": [torch.zeros(4)]}
    st.flat_grads.append(st.flat_ring["bufs"][0])
    st.bn_acc_buf, st.bn_acc_token = torch.zeros(2, dtype=torch.float64), object()
    st.owner, st.packs_fresh, st.counters_external = object(), True, True
    st.last_pass = _kept(torch.zeros(1), disc_graph.param_dict(m)[1])
    with st.keeping_pass((2, 1)), st.accumulating_grads() as scope:
        scope.flat = torch.zeros(4)
        assert listing() == before
    assert listing() == before
    for k, v in m.state_dict().items():
        assert torch.equal(v, values[k]), k


def test_scopes_restore_when_the_body_raises():
    st = state(torch.nn.Linear(2, 2))
    st.last_pass = object()
    with pytest.raises(ZeroDivisionError):
        with st.keeping_pass((2, 1)):
            assert st.keep_pass and st.arena_request == (2, 1) and st.last_pass is None
            1 / 0
    assert st.keep_pass is False and st.arena_request is None
    with pytest.raises(ZeroDivisionError):
        with st.external_counters():
            assert st.counters_external
            1 / 0
    assert st.counters_external is False
    with pytest.raises(ZeroDivisionError):
        with st.accumulating_grads() as scope:
            assert st.grad_accum is scope and scope.flat is None
            1 / 0
    assert st.grad_accum is None


def test_keeping_pass_leaves_the_kept_pass():
    st = state(torch.nn.Linear(2, 2))
    kept = object()
    with st.keeping_pass():
        assert st.arena_request is None
        st.last_pass = kept                 # what disc_graph.DiscriminatorFn does inside the scope
    assert st.last_pass is kept and st.keep_pass is False


def test_module_flat_grad_finds_the_buffer_of_the_views():
    from srganst import dist as sdist
    from srganst import ops
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    ps = list(model.parameters())
    assert sdist.module_flat_grad(model) is None                  # no state, no gradients
    offs, total = ops.flat_layout(ps)
    flat = torch.randn(total)
    for p, o in zip(ps, offs):
        p.grad = flat[o:o + p.numel()].view(p.shape)
    assert sdist.module_flat_grad(model) is None                  # views of a buffer the module does not know
    state(model).flat_grads += [torch.zeros(3), flat, torch.zeros(total)]
    assert sdist.module_flat_grad(model) is flat
    ps[1].grad = ps[1].grad.clone()
    assert sdist.module_flat_grad(model) is None


def test_kept_pass_is_pass_over():
    from srganst import disc_graph
    D = _small("D")
    names, pd = disc_graph.param_dict(D)
    assert names == [n for n, _ in D.named_parameters()] and list(pd) == names
    assert all(not pd[n].requires_grad and pd[n].data_ptr() == p.data_ptr() for n, p in D.named_parameters())
    x = torch.rand(2, 3, 8, 8)
    kept = _kept(x, pd)
    assert kept.is_pass_over(x, disc_graph.param_dict(D)[1], names)
    assert not kept.is_pass_over(x.clone(), disc_graph.param_dict(D)[1], names)         # another input
    assert not kept.is_pass_over(x[:1], disc_graph.param_dict(D)[1], names)             # same pointer, another shape
    w = D.features[0].weight
    with torch.no_grad():
        w.add_(1.0)                                                                     # modified through torch: _version moves
    assert not kept.is_pass_over(x, disc_graph.param_dict(D)[1], names)
    kept = _kept(x, disc_graph.param_dict(D)[1])
    assert kept.is_pass_over(x, disc_graph.param_dict(D)[1], names)
    w.data = w.data.clone()                                                             # rebound: another pointer
    assert not kept.is_pass_over(x, disc_graph.param_dict(D)[1], names)
