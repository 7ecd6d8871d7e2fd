"""Kernel graph of the SRResNet generator: forward and hand-written backward over srganst.ops.

Forward  = reference model.py:142-152 (+155-184), backward = what autograd derives from it.
Activations are NHWC; the NCHW surface is met by the first (transpose of the 3-channel LR input)
and last (conv3 stores NCHW + clamp) kernels.  Fusions relative to the reference's op list:
  * BatchNorm-apply + PReLU of a producer are applied while the consumer conv stages its input;
  * BatchNorm batch statistics are emitted by the conv epilogue (per-tile partials);
  * PixelShuffle is the up-conv's store pattern; clamp_ is conv3's store;
  * PReLU outputs are never materialised (pre-activation tensors are kept, the slope is re-applied on load).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops
from ._state import state
from .ops import ACT_SLOPE, OUT_NCHW_CLAMP, OUT_SHUFFLE


class _BN:
    """A BatchNorm between the conv that produces its input and the kernels that consume its output.  Eval mode fills only
    scale / shift.  Tile mode fills the four tensors with a bn_finalize launch right after the producer.  Accumulator mode
    allocates them empty (stats()): the producer adds into its fp64 accumulator row `acc`, and the first consumer - the next
    conv's prologue, or bn_finalize_acc ahead of a stand-alone kernel - fills them and moves the running statistics."""
    __slots__ = ("mod", "name", "gamma", "beta", "acc", "mean", "rstd", "scale", "shift")

    def __init__(self, mod, name, gamma, beta, acc=None):
        self.mod, self.name, self.gamma, self.beta, self.acc = mod, name, gamma, beta, acc     # name.weight / name.bias = gamma / beta
        self.mean = self.rstd = self.scale = self.shift = None

    def running(self):
        return self.mod.running_mean, self.mod.running_var

    def stats(self):
        self.mean, self.rstd, self.scale, self.shift = (ops._f32(self.gamma.numel(), like=self.gamma) for _ in range(4))
        return self.mean, self.rstd, self.scale, self.shift


@dataclass
class _Block:
    """Residual block: input h, y1 = conv_a(h), y2 = conv_b(PReLU(bn1(y1))); its output h + bn2(y2) is formed by the next conv."""
    h: torch.Tensor
    y1: torch.Tensor
    bn1: _BN
    y2: torch.Tensor
    bn2: _BN


@dataclass
class _Up:
    """Up-sampling stage: input u (a pre-activation when slope is given), us = PixelShuffle(conv(PReLU(u))).  conv3 is saved as
    one more stage: us = its output before the clamp."""
    u: torch.Tensor
    slope: torch.Tensor | None
    us: torch.Tensor | None


@dataclass
class _Saved:
    """What forward() keeps for backward()."""
    x3: torch.Tensor
    z1: torch.Tensor
    blocks: list
    h_last: torch.Tensor            # conv2's input (a pre-activation, z1, when there are no blocks)
    y3: torch.Tensor
    bn3: _BN
    ups: list
    last: _Up
    wd: dict | None                 # data-gradient packs, made by the forward's multi-tensor launch
    w9: dict
    fast9: bool
    acc_mode: bool
    acc_token: object = None        # accumulator mode: see _Accumulators


class _Accumulators:
    """The fp64 BatchNorm accumulators of the accumulator mode.  ONE buffer (HipState.bn_acc_buf) holds the forward rows
    [2*nblocks+1, NREP, C, 2] (sum, sum of squares per BatchNorm) and behind them the backward rows [2*nblocks, NREP, C, 4].
    The training forward clears the whole buffer with a rider on its pack launch (`buf` goes into the riders) and leaves a
    fresh token on HipState.bn_acc_token and in its saved record.  A backward that still finds its forward's token adds into
    the clear backward rows; any other (a second backward, or another forward in between) clears them again first.  Every
    backward drops the token: its rows are dirty from then on."""

    def __init__(self, module, nblocks, C, device):
        nf, nbk = (2 * nblocks + 1) * ops.ACC_NREP * C * 2, 2 * nblocks * ops.ACC_NREP * C * 4
        self.st = state(module)
        buf = self.st.bn_acc_buf
        if buf is None or buf.numel() != nf + nbk or buf.device != device:
            buf = self.st.bn_acc_buf = torch.zeros(nf + nbk, device=device, dtype=torch.float64)
        self.buf, self.nf = buf, nf
        self.fwd = buf[:nf].view(2 * nblocks + 1, ops.ACC_NREP, C, 2)
        self.bwd = buf[nf:].view(2 * nblocks, ops.ACC_NREP, C, 4)

    def new_token(self):
        self.st.bn_acc_token = token = object()
        return token

    def backward_rows(self, token):
        if token is None or self.st.bn_acc_token is not token:
            self.buf[self.nf:].zero_()
        self.st.bn_acc_token = None
        return self.bwd


def _act(slope):
    return ACT_SLOPE if slope is not None else 0


def _fast9(p):
    """The 9x9 convs take the (kx, 3ch)-folded kernels when their small side has exactly 3 channels (the reference's
    RGB configuration) and C is a multiple of 4 that the wgrad kernel supports."""
    C = p["conv1.0.weight"].shape[0]
    return p["conv1.0.weight"].shape[1] == 3 and p["conv3.weight"].shape[0] == 3 and ops.wgrad_c3_supported(C)


def _conv_names(module, fast9):
    names = [] if fast9 else ["conv1.0.weight"]
    for i in range(len(module.trunk)):
        names += [f"trunk.{i}.rcb.0.weight", f"trunk.{i}.rcb.3.weight"]
    names.append("conv2.0.weight")
    names += [f"upsampling.{j}.upsample_block.0.weight" for j in range(len(module.upsampling))]
    if not fast9:
        names.append("conv3.weight")
    return names


def _packs(module, p, fast9, with_dgrad, extras=()):
    """All packed weights of the generator from ONE multi-tensor launch: (forward packs by name, data-gradient packs by name or
    None, packs of the (kx, 3ch)-folded 9x9 kernels {"conv1", "conv3", "conv3.dgrad"}).  The data-gradient packs are made by
    the training forward and handed to backward() (the weights do not change in between).  extras: ops.PackPlan's riders."""
    cache = state(module).cache
    names = _conv_names(module, fast9)
    ws = [p[n] for n in names]
    modes = [ops.PACK_FWD] * len(ws)
    if with_dgrad:
        ws += [p[n] for n in names]
        modes += [ops.PACK_DGRAD] * len(names)
    nine = []
    if fast9:
        nine = [("conv1", "conv1.0.weight", ops.PACK_C3_FWD), ("conv3", "conv3.weight", ops.PACK_TO3)]
        if with_dgrad:
            nine.append(("conv3.dgrad", "conv3.weight", ops.PACK_C3_DGRAD))
        ws += [p[n] for _, n, _ in nine]
        modes += [m for _, _, m in nine]
    out = ops.packed_weights(cache, ("pack", bool(with_dgrad), tuple(e[0] for e in extras)), ws, modes, extras)
    k = len(names)
    wp = dict(zip(names, out[:k]))
    wd = dict(zip(names, out[k:2 * k])) if with_dgrad else None
    w9 = {key: t for (key, _, _), t in zip(nine, out[(2 * k if with_dgrad else k):])}
    return wp, wd, w9


def forward(module, x, params, need_grad):
    p = dict(zip(module._names, params))
    training = module.training
    C = p["conv1.0.weight"].shape[0]
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    nb = len(module.trunk)
    # accumulator mode: no BatchNorm finalize launches - each trunk conv adds its output statistics into fp64 accumulators and
    # the NEXT conv derives the affine of its input from them in its prologue (csrc/conv_epilogue.h: BandAcc)
    acc_mode = bool(training and nb and ops.conv_acc_supported(B, H, W, C, C))
    fast9 = _fast9(p)
    # the batch counters' add and the clearing of the statistics accumulators (two one-line launches at the head of the serial chain)
    # ride in the pack launch
    extras = []
    counters = ops.flatten_bn_counters(module) if training else None
    if counters is not None:
        extras.append(("add", counters, 1))
    if acc_mode:
        accs = _Accumulators(module, nb, C, x.device)
        extras.append(("zero", accs.buf))
    wp, wd, w9 = _packs(module, p, fast9, need_grad, tuple(extras))
    acc_token = accs.new_token() if acc_mode else None
    x3 = ops.transpose(x.contiguous(), to_nchw=False)                                  # [B,h,w,3]
    if fast9:
        z1 = ops.conv9_c3_fwd(x3, p["conv1.0.weight"], 0, bias=p["conv1.0.bias"], wp=w9["conv1"])
    else:
        z1, _, _, _ = ops.conv_fwd(x3, wp["conv1.0.weight"], C, 9, 1, bias=p["conv1.0.bias"])
    a1 = p["conv1.1.weight"]
    n_px = float(B * H * W)

    def link(mod, name, k):          # the k-th BatchNorm of the trunk
        return _BN(mod, name, p[name + ".weight"], p[name + ".bias"], accs.fwd[k] if acc_mode else None)

    def conv(t, w, out_bn, in_bn=None, slope=None, pend=None):
        """One trunk conv, its output statistics going to out_bn.  Input: PReLU_slope(in_bn(t)), or - pend, a _Block - that
        block's output pend.h + bn2(pend.y2), formed while staging.  -> (y, the input: t, or the sum just formed)."""
        src = pend.bn2 if pend else in_bn
        if acc_mode:
            kw = dict(in_acc=src.acc, in_bn=(src.gamma, src.beta), n=n_px, out_stats=src.stats(), run_stats=src.running()) if src else {}
            y, h = ops.conv_fwd_acc(pend.h if pend else t, w, C, 3, in2=pend.y2 if pend else None, in_slope=slope, in_act=_act(slope),
                                    st_acc=out_bn.acc, **kw)
        else:
            if pend:
                y, h, st, cnt = ops.conv_fwd_resin(pend.h, pend.y2, src.scale, src.shift, w, C, 3, want_stats=training)
            else:
                y, h, st, cnt = ops.conv_fwd(t, w, C, 3, 1, in_scale=src.scale if src else None, in_shift=src.shift if src else None,
                                             in_slope=slope, in_act=_act(slope), want_stats=training)
            if training:
                out_bn.mean, out_bn.rstd, out_bn.scale, out_bn.shift = ops.bn_finalize(st, cnt, out_bn.gamma, out_bn.beta, *out_bn.running())
            else:
                out_bn.scale, out_bn.shift = ops.bn_eval_affine(out_bn.gamma, out_bn.beta, *out_bn.running())
        return y, h if pend else t

    def materialise(bn):             # ahead of a stand-alone consumer (tile / eval mode: done right after the producer)
        if acc_mode:
            bn.mean, bn.rstd, bn.scale, bn.shift = ops.bn_finalize_acc(bn.acc, n_px, bn.gamma, bn.beta, *bn.running())

    h, slope = z1, a1     # slope: h is a pre-activation whose PReLU the consumer applies on load (z1 only)
    pend = None           # the previous block while its output h + bn2(y2) is not materialised yet: the next conv forms it while
    blocks = []           # staging its input and hands it back (one bn_residual launch less per block)
    for i, blk in enumerate(module.trunk):
        pre = f"trunk.{i}.rcb"
        bn1, bn2 = link(blk.rcb[1], pre + ".1", 2 * i), link(blk.rcb[4], pre + ".4", 2 * i + 1)
        y1, h = conv(h, wp[pre + ".0.weight"], bn1, slope=slope, pend=pend)
        y2, _ = conv(y1, wp[pre + ".3.weight"], bn2, in_bn=bn1, slope=p[pre + ".2.weight"])
        blocks.append(_Block(h, y1, bn1, y2, bn2))
        if i == 0:        # the skip term is PReLU(z1): stand-alone residual kernel for this one block
            materialise(bn2)
            h, slope = ops.bn_residual(y2, bn2.scale, bn2.shift, h, a1), None
        else:
            pend = blocks[-1]
    bn3 = link(module.conv2[1], "conv2.1", 2 * nb)
    y3, h = conv(h, wp["conv2.0.weight"], bn3, slope=slope, pend=pend)
    materialise(bn3)
    u = ops.bn_residual(y3, bn3.scale, bn3.shift, z1, a1)
    ups = []
    slope = None
    for j, _ in enumerate(module.upsampling):
        pre = f"upsampling.{j}.upsample_block"
        us, _, _, _ = ops.conv_fwd(u, wp[pre + ".0.weight"], 4 * C, 3, 1, bias=p[pre + ".0.bias"],
                                   in_slope=slope, in_act=_act(slope), out_mode=OUT_SHUFFLE)
        ups.append(_Up(u, slope, us))
        u, slope = us, p[pre + ".2.weight"]
    if fast9:
        sr, sr_pre = ops.conv9_to3_fwd(u, p["conv3.weight"], bias=p["conv3.bias"], in_slope=slope, in_act=_act(slope),
                                       want_pre=need_grad, wp=w9["conv3"])
    else:
        sr, sr_pre, _, _ = ops.conv_fwd(u, wp["conv3.weight"], p["conv3.weight"].shape[0], 9, 1, bias=p["conv3.bias"], in_slope=slope,
                                        in_act=_act(slope), out_mode=OUT_NCHW_CLAMP, want_pre=need_grad)
    return sr, _Saved(x3, z1, blocks, h, y3, bn3, ups, _Up(u, slope, sr_pre), wd, w9, fast9, acc_mode, acc_token)


def backward(module, params, sv, dsr, need_dx=False):
    """-> list of gradients in module._names order."""
    p = dict(zip(module._names, params))
    grads = ops.flat_grads(module, module._names, params)      # views of ONE flat buffer (single RCCL message)
    C = p["conv1.0.weight"].shape[0]
    a1 = p["conv1.1.weight"]
    wd, w9, fast9 = sv.wd, sv.w9, sv.fast9
    wg = ops.WgradGroup()            # the trunk-shaped weight gradients go out as ONE launch at the end

    # ---- conv3 + clamp
    u, slope = sv.last.u, sv.last.slope
    g3 = ops.clamp_bwd(dsr.contiguous(), sv.last.us, dbias=grads["conv3.bias"])
    with ops.SideStream(u, g3, grads["conv3.weight"]):      # a weight gradient: a leaf of the backward chain
        if fast9:
            ops.wgrad_c3(u, g3, grads["conv3.weight"], 0, in_slope=slope, in_act=_act(slope))
        else:
            ops.conv_wgrad(u, g3, grads["conv3.weight"], 9, 1, in_slope=slope, in_act=_act(slope))
    if fast9:
        g = ops.conv9_c3_fwd(g3, p["conv3.weight"], 1, wp=w9["conv3.dgrad"])              # d PReLU(u)
    else:
        g = ops.conv_fwd(g3, wd["conv3.weight"], C, 9, 1)[0]
    # ---- up-sampling blocks, last to first
    for j, up in reversed(list(enumerate(sv.ups))):
        pre = f"upsampling.{j}.upsample_block"
        # PReLU backward + inverse PixelShuffle + the partial sums of (conv bias, slope) gradients in ONE pass, one finalize
        du = ops.act_bwd(g, up.us, slope=p[pre + ".2.weight"], dbias=grads[pre + ".0.bias"], dslope=grads[pre + ".2.weight"],
                         unshuffle=True)                                             # [B,h,w,4C] pre-shuffle grad
        with ops.SideStream(up.u, du, grads[pre + ".0.weight"]):
            ops.conv_wgrad(up.u, du, grads[pre + ".0.weight"], 3, 1, in_slope=up.slope, in_act=_act(up.slope))
        g = ops.conv_fwd(du, wd[pre + ".0.weight"], C, 3, 1)[0]    # d (input of the up-conv)
    # ---- u = BN(conv2(h_last)) + PReLU(z1)
    y3, bn3, blocks = sv.y3, sv.bn3, sv.blocks
    nb = len(blocks)
    n = y3.numel() // y3.shape[-1]
    dy3 = ops.bwd_reduce_apply(g, y3, n, scale=bn3.scale, shift=bn3.shift, mean=bn3.mean, rstd=bn3.rstd, gamma=bn3.gamma,
                               dgamma=grads["conv2.1.weight"], dbeta=grads["conv2.1.bias"])
    wg.add(sv.h_last, dy3, grads["conv2.0.weight"], 3, 1, in_slope=None if nb else a1, in_act=0 if nb else ACT_SLOPE)
    dskip = g
    # Every trunk data-gradient conv also emits the BatchNorm-backward sums of its result against the conv output the NEXT stage
    # differentiates through.  Tile mode: per-tile partials (`part`), a bwd_finalize launch ahead of each stage.  Accumulator mode:
    # fp64 accumulator rows (bacc), each stage derives its coefficients from them in its prologue.
    bacc = _Accumulators(module, nb, C, y3.device).backward_rows(sv.acc_token) if sv.acc_mode else None
    part = None
    if not nb:
        dh = ops.conv_fwd(dy3, wd["conv2.0.weight"], C, 3, 1)[0]
    elif sv.acc_mode:
        dh, _ = ops.conv_dgrad_fused_acc(dy3, wd["conv2.0.weight"], C, 3, epi_y=blocks[-1].y2, bw_st_acc=bacc[2 * nb - 1])
    else:
        dh, part = ops.conv_dgrad_bwdstats(dy3, wd["conv2.0.weight"], C, 3, blocks[-1].y2)

    def stage(g, y, bn, k, w, part, epi_y, dslope=None, **kw):
        """One BatchNorm-backward stage: dy = g through bn (the k-th of the trunk) against its input y, out = data-gradient conv
        of dy, with the sums of `out` against epi_y (if any) for the next stage, BatchNorm k - 1.  -> (out, dy, part)."""
        dgamma, dbeta = grads[bn.name + ".weight"], grads[bn.name + ".bias"]
        if sv.acc_mode:
            out, dy = ops.conv_dgrad_fused_acc(g, w, C, 3, y2=y, epi_y=epi_y, bw_in_acc=bacc[k], bn=(bn.mean, bn.rstd, bn.gamma), n=n,
                                               dgamma=dgamma, dbeta=dbeta, dslope=dslope,
                                               bw_st_acc=None if epi_y is None else bacc[k - 1], **kw)
            return out, dy, None
        cA, cB, cC = ops.bwd_finalize(part, n, bn.mean, bn.rstd, bn.gamma, dgamma, dbeta, dslope=dslope)
        return ops.conv_dgrad_fused(g, y, w, C, 3, cA, cB, cC, epi_y=epi_y, **kw)

    # ---- residual blocks, last to first
    for i, b in reversed(list(enumerate(blocks))):
        pre = f"trunk.{i}.rcb"
        s1, t1, sl = b.bn1.scale, b.bn1.shift, p[pre + ".2.weight"]
        # stage 2 (BN2, no activation)
        dp1, dy2, part = stage(dh, b.y2, b.bn2, 2 * i + 1, wd[pre + ".3.weight"], part, b.y1,
                               epi_scale=s1, epi_shift=t1, epi_slope=sl, epi_act=1)
        wg.add(b.y1, dy2, grads[pre + ".3.weight"], 3, 1, in_scale=s1, in_shift=t1, in_slope=sl, in_act=ACT_SLOPE)
        # stage 1 (BN1 + PReLU); its sums are against y2 of the block before
        dh, dy1, part = stage(dp1, b.y1, b.bn1, 2 * i, wd[pre + ".0.weight"], part, blocks[i - 1].y2 if i else None,
                              dslope=grads[pre + ".2.weight"], in_scale=s1, in_shift=t1, in_slope=sl, in_act=ACT_SLOPE, residual=dh)
        wg.add(b.h, dy1, grads[pre + ".0.weight"], 3, 1, in_slope=None if i else a1, in_act=0 if i else ACT_SLOPE)
    # ---- c1 = PReLU(z1): gradient = trunk path (dh) + global skip (dskip)
    dz1 = ops.act_bwd(dh, sv.z1, g2=dskip, slope=a1, dbias=grads["conv1.0.bias"], dslope=grads["conv1.1.weight"])
    with ops.SideStream(dz1, sv.x3, grads["conv1.0.weight"]):
        if fast9:
            ops.wgrad_c3(dz1, sv.x3, grads["conv1.0.weight"], 1)
        else:
            ops.conv_wgrad(sv.x3, dz1, grads["conv1.0.weight"], 9, 1)
    wg.run()
    ops.join_side()
    dx = None
    if need_dx:
        wd1 = ops.pack_conv(p["conv1.0.weight"], 1) if fast9 else wd["conv1.0.weight"]
        dx3 = ops.conv_fwd(dz1, wd1, sv.x3.shape[-1], 9, 1)[0]
        dx = ops.transpose(dx3, to_nchw=True)
    return [grads[n] for n in module._names], dx


class GeneratorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, grad_mode, *params):
        need_grad = grad_mode and any(ctx.needs_input_grad)
        if need_grad and not module.training:
            raise NotImplementedError("Generator backward in eval() mode is not on the reference's path "
                                      "(train.py:109 / warmup.py:71 call .train() before every epoch)")
        sr, sv = forward(module, x, [t.detach() for t in params], need_grad)
        if need_grad:
            ctx.module, ctx.sv, ctx.params = module, sv, [t.detach() for t in params]
            ctx.need_dx = ctx.needs_input_grad[0]
        return sr

    @staticmethod
    def backward(ctx, dsr):
        grads, dx = backward(ctx.module, ctx.params, ctx.sv, dsr, ctx.need_dx)
        ctx.sv = None
        return (dx, None, None, *grads)
