"""Kernel graph of the VGG-style discriminator: forward and hand-written backward over srganst.ops.

Forward = reference model.py:67-71 over the layer list model.py:30-65; backward = what autograd
derives.  NHWC activations; conv outputs are kept pre-BatchNorm / pre-activation and the
BN-apply + LeakyReLU(0.2) is fused into the consumer's load.  The flatten (model.py:69) keeps the
reference's (C,H,W) order so classifier.0.weight is used in its reference layout.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import torch

from . import ops
from ._state import KeptPass, state
from .ops import ACT_SLOPE

LRELU = 0.2

# (conv index, bn index or None, stride) in module.features                           model.py:30-59
PLAN = [(0, None, 1), (2, 3, 2), (5, 6, 1), (8, 9, 2), (11, 12, 1), (14, 15, 2), (17, 18, 1), (20, 21, 2)]


class _Layer:
    """One conv [+ BatchNorm] + LeakyReLU stage of a pass: its row of PLAN and the conv's output y (pre-BatchNorm, pre-activation).
    A BatchNorm stage adds the affine its consumers apply on load (scale, shift; eval mode stops there), the batch statistics the
    backward needs (mean, rstd) and the conv's per-tile partials (st, cnt) that replay_running_stats finalizes once more.  Over
    passes batched as one tall image the four vectors are [passes, C] tables.  The stage's input is not kept: _Saved.input_of."""
    __slots__ = ("ci", "bi", "stride", "y", "mean", "rstd", "scale", "shift", "st", "cnt")

    def __init__(self, ci, bi, stride, y, mean=None, rstd=None, scale=None, shift=None):
        self.ci, self.bi, self.stride, self.y = ci, bi, stride, y
        self.mean, self.rstd, self.scale, self.shift, self.st, self.cnt = mean, rstd, scale, shift, None, None

    def epi(self, prefix=""):
        """LeakyReLU([BatchNorm](y)) as the keyword arguments of a kernel that differentiates through it."""
        return {prefix + "y": self.y, prefix + "scale": self.scale, prefix + "shift": self.shift, prefix + "slope_const": LRELU,
                prefix + "act": 1}


@dataclass
class _Saved:
    """What forward() keeps of one pass for backward() - or of `groups` passes of gB images each run (or, PassArena.all_slots, laid
    out) as one batch; a single pass has groups = 1, gB = 0.  x3 is the NHWC input, flat / h1 the classifier's input and its hidden
    pre-activation, wd / ws2 the stride-1 / stride-2 data-gradient packs by name (None when the forward ran without gradients)."""
    x3: torch.Tensor
    layers: list
    flat: torch.Tensor | None
    h1: torch.Tensor | None
    groups: int
    gB: int
    wd: dict | None
    ws2: dict | None

    def input_of(self, li):
        """(input tensor of layer li, the in_* keyword arguments that apply the stage below on load): x3 as it is for the bottom layer."""
        if li == 0:
            return self.x3, dict(in_scale=None, in_shift=None, in_slope_const=LRELU, in_act=0)
        r = self.layers[li - 1]
        return r.y, dict(in_scale=r.scale, in_shift=r.shift, in_slope_const=LRELU, in_act=ACT_SLOPE)


# HipState.cache["pack_state"]: the packs made from the parameter values sig = ((data_ptr, _version) per conv weight)
_Packs = namedtuple("_Packs", "sig wp wd ws2")


class _GradSink:
    """Where one backward pass puts its parameter gradients: per-parameter views of ONE flat buffer, and whether the pass accumulates
    into it - the second and later passes inside an accumulation scope do (HipState.grad_accum).  take(name) hands a kernel its view
    and counts it as produced.  g carries d LeakyReLU(BN(y_last)) (NHWC) from backward_classifier to backward_features."""
    __slots__ = ("views", "acc", "taken", "g")

    def __init__(self, module, p, need_param_grads):
        names = list(p.keys())
        hs = state(module)
        scope = hs.grad_accum if need_param_grads else None
        self.acc = scope is not None and scope.flat is not None
        if self.acc:
            plist = [p[n] for n in names]
            offs, _ = ops.flat_layout(plist)
            self.views = {n: scope.flat[o:o + t.numel()].view(t.shape) for n, t, o in zip(names, plist, offs)}
        else:
            self.views = ops.flat_grads(module, names, [p[n] for n in names]) if need_param_grads else {}
            if scope is not None:
                scope.flat = hs.flat_grads[-1]
        self.taken, self.g = {}, None

    def take(self, name):
        t = self.taken[name] = self.views[name]
        return t

    def grads(self):
        return {} if self.acc else self.taken      # by name; none from a pass that added into the first pass's buffer


def param_dict(module):
    """(parameter names in the reference's order, {name: detached parameter}): what the functions below take as `p`."""
    names = [n for n, _ in module.named_parameters()]
    return names, dict(zip(names, [t.detach() for t in module.parameters()]))


def packs(module, p, with_dgrad, counter_add=0):
    """(forward packs by name, stride-1 data-gradient packs by name, stride-2 data-gradient packs by name) - the last two None
    without with_dgrad.  One multi-tensor launch + one launch per stride-2 layer, or none: while the module has an owner and its
    packs are fresh they are handed out again (HipState.owner).
    counter_add > 0 (the owner's call at the head of an iteration, which always packs): the BatchNorm batch counters' add for the
    iteration's passes rides in the pack launch."""
    hs = state(module)
    cache = hs.cache
    names = [f"features.{ci}.weight" for ci, _, _ in PLAN]
    n1, n2 = ([n for n, (_, _, s) in zip(names, PLAN) if s == stride] for stride in (1, 2))
    sig = tuple((p[n].data_ptr(), p[n]._version) for n in names)
    st = cache.get("pack_state")
    if hs.owner is not None and hs.packs_fresh and st is not None and st.sig == sig and (st.wd is not None or not with_dgrad):
        assert not counter_add, "the packs are fresh: nothing to ride along with"
        return st.wp, st.wd, st.ws2
    ws = [p[n] for n in names] + ([p[n] for n in n1] if with_dgrad else [])
    modes = [ops.PACK_FWD] * len(names) + ([ops.PACK_DGRAD] * len(n1) if with_dgrad else [])
    extras = (("add", ops.flatten_bn_counters(module), int(counter_add)),) if counter_add else ()
    out = ops.packed_weights(cache, ("pack", bool(with_dgrad), int(counter_add)), ws, modes, extras)
    wp = dict(zip(names, out[:len(names)]))
    wd = ws2 = None
    if with_dgrad:
        wd = dict(zip(n1, out[len(names):]))
        ws2 = {n: ops.pack_conv_s2_dgrad(p[n], out=cache.get(("s2", n))) for n in n2}
        for n in n2:
            cache[("s2", n)] = ws2[n]
    cache["pack_state"] = _Packs(sig, wp, wd, ws2)
    hs.packs_fresh = True
    return wp, wd, ws2


def groups_supported(module, p, gB, groups, H, W):
    """Can `groups` passes of gB images each (H x W) run as ONE batch with per-pass BatchNorm statistics?  Every BatchNorm layer's
    producer and consumer must be on the kernels that take coefficient groups (the pipelined conv, the all-taps weight gradient)."""
    B = gB * groups
    h, w = H, W
    for li, (ci, bi, stride) in enumerate(PLAN):
        wt = p[f"features.{ci}.weight"]
        cout, cin = wt.shape[0], wt.shape[1]
        if li > 0 and not (ops.conv_pipe_groups_ok(B, h, w, cin, cout, 3, stride, gB)
                           and (stride != 1 or ops.conv_pipe_groups_ok(B, h, w, cout, cin, 3, 1, gB))      # its data-gradient (epilogue partials)
                           and ops.conv_wgrad_groups_ok(B, h, w, cin, cout, 3, stride, gB)):
            return False
        h, w = ops.conv_out_hw(h, w, 3, stride)
    return B <= 64            # classifier kernels: at most 64 batch rows


class PassArena:
    """Activations of several passes side by side: every tensor the backward reads is allocated once for `slots` passes of B images
    and each pass's forward (slot = its place) writes its part.  Passes that ran separately - the generator step's D(sr) and, later,
    the discriminator step's D(gt) (engine.TrainEngine with KERNEL.REUSE_D_SR) - can then be differentiated as ONE batch
    (all_slots): per-pass BatchNorm rows, one launch per layer over slots * B images.
    x3, flat, h1 and y[li] are [slots * B, ...]; bn[li] is [4, slots, C]: the mean, rstd, scale and shift tables of a BatchNorm layer."""

    def __init__(self, slots):
        self.slots, self.B, self.filled = slots, None, set()
        self.x3 = self.flat = self.h1 = None
        self.y, self.bn = [None] * len(PLAN), [None] * len(PLAN)

    def part(self, slot, name, li, shape, like):
        """What the pass in `slot` writes of "x3" / "flat" / "h1" (li None) or of "y" / "bn" of layer li; all slots are allocated when
        the first pass asks.  shape is ONE pass's: [B, ...] -> the slot's B images; (C,) for "bn" -> its row of each of the four tables."""
        if name != "bn":
            self.B = self.B or shape[0]
            assert shape[0] == self.B, "every pass of an arena has the same batch size"
        held, key = (self.__dict__, name) if li is None else (getattr(self, name), li)
        if held[key] is None:
            full = (4, self.slots, *shape) if name == "bn" else (self.slots * shape[0], *shape[1:])
            held[key] = torch.empty(full, device=like.device, dtype=torch.float32)
        return tuple(held[key][:, slot]) if name == "bn" else held[key][slot * self.B:(slot + 1) * self.B]

    def all_slots(self, sv):
        """The saved record of all `slots` passes as one batch (what forward() on a list of inputs would have saved), once every slot
        has been filled by a forward(..., arena=(arena, slot)) of the same weights; `sv`: any of those passes (for its packs)."""
        assert len(self.filled) == self.slots, "not every pass of the arena has run"
        layers = [_Layer(ci, bi, stride, self.y[li], *(self.bn[li] if bi is not None else ())) for li, (ci, bi, stride) in enumerate(PLAN)]
        return _Saved(self.x3, layers, self.flat, self.h1, self.slots, self.B, sv.wd, sv.ws2)


def forward(module, x, p, training, need_grad=False, arena=None):
    """x: one NCHW batch, or a LIST of `groups` equally-shaped NCHW batches = that many passes of the discriminator run as ONE
    batch (each pass keeps its own train-mode BatchNorm statistics: per-pass scale / shift rows, running statistics updated pass by
    pass in list order, batch counters + groups) - the discriminator step's D(gt) and D(sr.detach()) (train.py:155-158) as one tall
    image; returns logits [groups * B, 1] and the _Saved record."""
    groups, gB = 1, 0
    ar, slot = arena if arena is not None else (None, 0)      # (PassArena, slot): this pass writes its part of the shared tensors
    assert ar is None or (training and not isinstance(x, (list, tuple)))
    if isinstance(x, (list, tuple)):
        groups, gB = len(x), x[0].shape[0]
        if groups == 1:
            x, gB = x[0], 0
        elif not training:
            raise NotImplementedError("batched passes are a train-mode schedule (eval mode has no per-pass statistics to keep apart)")
    wp, wd, ws2 = packs(module, p, need_grad)
    if training and not state(module).counters_external:
        ops.flatten_bn_counters(module).add_(groups)
    if groups > 1:
        _, c3, hh, ww = x[0].shape
        x3 = torch.empty(groups * gB, hh, ww, c3, device=x[0].device, dtype=torch.float32)
        for gi, xi in enumerate(x):
            assert xi.shape == x[0].shape
            ops.transpose(xi.contiguous(), to_nchw=False, out=x3[gi * gB:(gi + 1) * gB])
    else:
        Bq, c3, hh, ww = x.shape
        x3 = ops.transpose(x.contiguous(), to_nchw=False, out=ar and ar.part(slot, "x3", None, (Bq, hh, ww, c3), x))
    sv = _Saved(x3, [], None, None, groups, gB, wd, ws2)
    for li, (ci, bi, stride) in enumerate(PLAN):
        h, in_kw = sv.input_of(li)
        cout = p[f"features.{ci}.weight"].shape[0]
        ho, wo = ops.conv_out_hw(h.shape[1], h.shape[2], 3, stride)
        y, _, st, cnt = ops.conv_fwd(h, wp[f"features.{ci}.weight"], cout, 3, stride, bias=p.get(f"features.{ci}.bias"), **in_kw,
                                     want_stats=(bi is not None and training), grp=gB,
                                     out=ar and ar.part(slot, "y", li, (h.shape[0], ho, wo, cout), h))
        rec = _Layer(ci, bi, stride, y)
        if bi is not None:
            bn = module.features[bi]
            g, b = p[f"features.{bi}.weight"], p[f"features.{bi}.bias"]
            if training:
                rec.mean, rec.rstd, rec.scale, rec.shift = ops.bn_finalize(st, cnt, g, b, bn.running_mean, bn.running_var, groups=groups,
                                                                           out=ar and ar.part(slot, "bn", li, (cout,), h))
                rec.st, rec.cnt = st, cnt
            else:
                rec.scale, rec.shift = ops.bn_eval_affine(g, b, bn.running_mean, bn.running_var)
        sv.layers.append(rec)
    h, w0 = rec.y, p["classifier.0.weight"]
    sv.flat = ops.flatten_act(h, rec.scale, rec.shift, LRELU, 1, grp=gB,                              # [B, C*H*W]  (C,H,W) order
                              out=ar and ar.part(slot, "flat", None, (h.shape[0], h[0].numel()), h))
    sv.h1 = ops.linear_fwd(sv.flat, w0, p["classifier.0.bias"], out=ar and ar.part(slot, "h1", None, (h.shape[0], w0.shape[0]), h))   # pre-activation
    if ar is not None:
        ar.filled.add(slot)
    return ops.head_fwd(sv.h1, p["classifier.2.weight"], p["classifier.2.bias"], LRELU), sv


def replay_running_stats(module, p, sv):
    """The side effects of ONE MORE train-mode forward over the input and weights of the pass saved in `sv`, without running it:
    every kernel of the forward is deterministic, so the second pass would reproduce the saved activations bit for bit - all it
    would add is one more step of the BatchNorm running statistics (same batch statistics: bn_finalize again on the saved
    per-tile partials, i.e. the very launch the forward would issue) and of num_batches_tracked.  engine.TrainEngine uses it for
    the discriminator step's D(sr.detach()) (train.py:158), which repeats the generator step's D(sr) (train.py:136) before any
    weight has changed."""
    if not state(module).counters_external:
        ops.flatten_bn_counters(module).add_(sv.groups)
    for rec in sv.layers:
        if rec.bi is None:
            continue
        bn = module.features[rec.bi]
        ops.bn_finalize(rec.st, rec.cnt, p[f"features.{rec.bi}.weight"], p[f"features.{rec.bi}.bias"],
                        bn.running_mean, bn.running_var, groups=sv.groups)


def backward_classifier(module, p, sv, dout, need_param_grads):
    """Backward of the classifier (model.py:61-65) of one pass: fills classifier.* gradients, returns the _GradSink the feature-stack
    half continues with.  The data-parallel engine runs this half of both passes first, so that the classifier bucket (75.5 MB) can
    be all-reduced while the feature stack's backward runs."""
    sink = _GradSink(module, p, need_param_grads)
    wg, acc = need_param_grads, sink.acc
    dh1 = ops.head_bwd(sv.h1, p["classifier.2.weight"], dout.contiguous(), LRELU, dw=sink.take("classifier.2.weight") if wg else None,
                       db=sink.take("classifier.2.bias") if wg else None, accumulate=acc)
    if wg:
        dw0, db0 = sink.take("classifier.0.weight"), sink.take("classifier.0.bias")
        with ops.SideStream(dh1, sv.flat, dw0, db0):
            ops.linear_wgrad(dh1, sv.flat, dw0, db0, accumulate=acc)
    B, H, W, C = sv.layers[-1].y.shape
    sink.g = ops.linear_dgrad(dh1, p["classifier.0.weight"], nhwc=(C, H * W)).view(B, H, W, C)
    return sink


def _bn_act_bwd(part, g, n, **kw):
    """dy through [BatchNorm ->] LeakyReLU; `part`: the reduction's partials where the data-gradient that produced g emitted them."""
    return ops.bwd_finalize_apply(part, g, n=n, **kw) if part is not None else ops.bwd_reduce_apply(g, n=n, **kw)


def backward_features(module, p, sv, sink, need_param_grads, need_dx, defer_wgrad=None, defer_below=None):
    """Backward of the feature stack (model.py:30-59) of one pass, continuing from backward_classifier's sink; returns (the
    pass's parameter gradients by name, dx or None).
    defer_wgrad (a list): the conv weight gradients are not launched here - they are leaves of the backward chain (nothing in this
    pass reads them) - but appended as (event recorded on the current stream once dy exists, launch closure); the caller runs them
    wherever the chip has room (engine.TrainEngine._iter_gd: on the generator's stream once its backward is done).  defer_below: only
    the layers with index < defer_below (the ones the chain reaches last) are deferred."""
    wg, acc, g = need_param_grads, sink.acc, sink.g
    groups, gB = sv.groups, sv.gB    # passes batched as one tall image: per-pass coefficient rows
    dx = part = None                 # part: BN/activation backward partials of g, when the producing dgrad conv emitted them
    reduces = [] if ops.WGRAD_REDUCE_MULTI else None      # slab reduces left for one launch at the end of the pass
    for li in reversed(range(len(sv.layers))):
        r, below = sv.layers[li], sv.layers[li - 1] if li > 0 else None
        x, in_kw = sv.input_of(li)
        n = r.y.numel() // r.y.shape[-1] // groups      # elements per channel of ONE pass (each has its own batch statistics)
        wname = f"features.{r.ci}.weight"
        cin = p[wname].shape[1]
        if r.bi is not None:
            gam = p[f"features.{r.bi}.weight"]
            dg = sink.take(f"features.{r.bi}.weight") if wg else torch.empty_like(gam)
            db = sink.take(f"features.{r.bi}.bias") if wg else torch.empty_like(gam)
            dy = _bn_act_bwd(part, g, n, **r.epi(), mean=r.mean, rstd=r.rstd, gamma=gam, dgamma=dg, dbeta=db, accumulate=acc and wg,
                             groups=groups)
        elif wg:
            dy = _bn_act_bwd(part, g, n, **r.epi(), dbeta=sink.take(f"features.{r.ci}.bias"), accumulate=acc, groups=groups)
        else:
            dy = ops.bwd_apply(g, **r.epi(), groups=groups)
        part = None
        if wg:
            dwc = sink.take(wname)

            def launch(x=x, dy=dy, dwc=dwc, stride=r.stride, in_kw=in_kw, red=None):
                ops.conv_wgrad(x, dy, dwc, 3, stride, **in_kw, accumulate=acc, grp=gB, defer_reduce=red)
            if defer_wgrad is not None and (defer_below is None or li < defer_below):
                ev = torch.cuda.Event()
                ev.record()
                defer_wgrad.append((ev, launch, (x, dy, dwc, in_kw["in_scale"], in_kw["in_shift"])))
            else:
                with ops.SideStream(x, dy, dwc):
                    launch(red=reduces)
        if li == 0 and not need_dx:
            break
        if r.stride == 1:
            if below is not None:    # g differentiates through the layer below's BN + LeakyReLU: emit its partials here
                g, part = ops.conv_dgrad_bwdstats(dy, sv.wd[wname], cin, 3, **below.epi("epi_"), grp=gB)
            else:
                g = ops.conv_fwd(dy, sv.wd[wname], cin, 3, 1)[0]
        else:
            # the backward partials of g against the layer below come out of the data-gradient's epilogue where the pipelined kernel
            # takes the shape (no separate reduce pass over g and y); they are only needed when the layer below has a BatchNorm
            # or parameter gradients are wanted (its bias)
            epi = below.epi() if below is not None and (below.bi is not None or wg) else None
            out = ops.conv_s2_dgrad(dy, sv.ws2[wname], x.shape[1], x.shape[2], cin, epi=epi, grp=gB)
            g, part = out if epi is not None else (out, None)
        if li == 0:
            dx = ops.transpose(g, to_nchw=True)
    if reduces:
        # the weight gradients' slab reduces (leaves of the chain), all layers in one launch - on the stream the weight gradients ran on
        with ops.SideStream(*[t for j in reduces for t in j[:2]]):
            ops.wgrad_reduce_flush(reduces)
    ops.join_side()
    return sink.grads(), dx


def backward(module, p, sv, dout, need_param_grads, need_dx):
    sink = backward_classifier(module, p, sv, dout, need_param_grads)
    return backward_features(module, p, sv, sink, need_param_grads, need_dx)


class DiscriminatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, grad_mode, *params):
        names, p = param_dict(module)                # (`params` are module.parameters(), handed in for autograd to see them)
        need_param = grad_mode and any(ctx.needs_input_grad[3:])
        need_dx = grad_mode and ctx.needs_input_grad[0]
        need_grad = need_param or need_dx
        if need_grad and not module.training:
            raise NotImplementedError("Discriminator backward in eval() mode is not on the reference's path (train.py:110)")
        hs = state(module)
        keep = hs.keep_pass and need_grad and module.training
        req = hs.arena_request if keep else None          # (slots, slot): write this pass into a fresh PassArena
        arena = (PassArena(req[0]), req[1]) if req is not None else None
        out, sv = forward(module, x, p, module.training, need_grad, arena=arena)
        if keep:
            # the step engine re-uses this pass (replay_running_stats): input identity, logits, saved activations
            hs.last_pass = KeptPass(x.data_ptr(), tuple(x.shape), out, sv, p, arena[0] if arena is not None else None)
        if need_grad:
            ctx.module, ctx.sv, ctx.p, ctx.names = module, sv, p, names
            ctx.need_param, ctx.need_dx = need_param, need_dx
        return out

    @staticmethod
    def backward(ctx, dout):
        grads, dx = backward(ctx.module, ctx.p, ctx.sv, dout, ctx.need_param, ctx.need_dx)
        ctx.sv = None
        return (dx, None, None, *[grads.get(n) for n in ctx.names])
