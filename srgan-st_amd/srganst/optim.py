"""Adam on flat buffers: torch.optim.Adam's interface and state layout, one HIP kernel per step.

The reference builds ``optim.Adam(params, lr, betas, eps, weight_decay)`` (train.py:62-75, warmup.py:34-40) and steps LR
schedulers on it.  FlatAdam IS a torch.optim.Adam (schedulers, ``param_groups``, ``state_dict()`` / ``load_state_dict()``
keep working and checkpoints stay interchangeable); what changes is where the numbers live: parameters, gradients and
both moments are flat fp32 buffers of one layout, so ``step()`` is a single streaming pass (csrc/optim.hip) instead of
torch's multi-tensor launches (measured 130 us -> ~12 us per generator step on MI355X).

With ``ema_decay > 0`` the same pass also keeps an exponential moving average of the parameters in a flat buffer of the
parameters' layout (``ema``): ema <- d * ema + (1 - d) * p_new, d = ema_decay or, with ``ema_warmup``,
min(ema_decay, (1 + t) / (10 + t)) at Adam step t.  The average is NOT part of ``state_dict()`` (that stays torch's
layout); it travels as the state dict of a module whose parameters are views of the buffer (engine: ``g_ema``)."""
from __future__ import annotations

import torch

from . import ops
from ._state import state


class FlatAdam(torch.optim.Adam):
    def __init__(self, module, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, ema_decay=0.0,
                 ema_warmup=True, ema_buffer=None):
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        flat, offs, params = ops.flatten_params(module)
        dev = flat.device
        self._lr_dev = torch.tensor(float(lr), device=dev, dtype=torch.float32)
        # capturable: param_groups[0]["lr"] IS the device tensor (schedulers fill_() it, a captured graph sees the new value)
        super().__init__(params, lr=self._lr_dev if capturable else float(lr), betas=betas, eps=eps,
                         weight_decay=weight_decay, fused=True, capturable=capturable)
        self._module = module
        self._flat_p, self._offs, self._params = flat, offs, params
        self._m = torch.zeros_like(flat)
        self._v = torch.zeros_like(flat)
        self._steps = torch.zeros(len(params), device=dev, dtype=torch.float32)
        self._adopt_state()
        # the average: allocated and filled here, so it exists before any graph capture.  ema_buffer: a flat buffer of the same
        # layout that the caller owns (the flattened parameters of a shadow module) - the ONE buffer the kernel writes
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.ema = None
        if self.ema_decay > 0.0:
            if ema_buffer is not None and (ema_buffer.shape != flat.shape or ema_buffer.device != dev or ema_buffer.dtype != flat.dtype
                                           or not ema_buffer.is_contiguous()):
                raise ValueError("ema_buffer must be a contiguous fp32 buffer of the flat parameters' size on their device")
            self.ema = ema_buffer if ema_buffer is not None else torch.empty_like(flat)
            self.reset_ema()

    @torch.no_grad()
    def reset_ema(self):
        """The average starts over from the parameters as they are now (for callers that load weights after construction)."""
        if self.ema is not None:
            self.ema.copy_(self._flat_p)

    def _adopt_state(self):
        """(Re)build the per-parameter state entries torch's Adam expects, as views of the flat buffers."""
        for i, (p, o) in enumerate(zip(self._params, self._offs)):
            n = p.numel()
            self.state[p] = {"step": self._steps[i], "exp_avg": self._m[o:o + n].view(p.shape),
                             "exp_avg_sq": self._v[o:o + n].view(p.shape)}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)          # torch casts / moves the loaded tensors into self.state
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self._params, self._offs)):
                st = self.state.get(p)
                if not st:
                    continue
                n = p.numel()
                self._m[o:o + n].view(p.shape).copy_(st["exp_avg"])
                self._v[o:o + n].view(p.shape).copy_(st["exp_avg_sq"])
                self._steps[i] = float(st["step"])
        self._adopt_state()
        g = self.param_groups[0]
        if isinstance(g["lr"], torch.Tensor):          # keep OUR device scalar as the group's lr
            self._lr_dev.fill_(float(g["lr"]))
            g["lr"] = self._lr_dev

    def _flat_grad(self):
        """The flat gradient buffer when every p.grad is the flat_grads view of its parameter, else None."""
        g0 = self._params[0].grad
        if g0 is None:
            return None
        n = self._flat_p.numel()
        for cand in reversed(state(self._module).flat_grads):
            b = cand.data_ptr()
            if cand.numel() != n or g0.data_ptr() != b + 4 * self._offs[0]:
                continue
            pb = self._flat_p.data_ptr()
            if all(p.grad is not None and p.grad.data_ptr() == b + 4 * o and p.data_ptr() == pb + 4 * o
                   for p, o in zip(self._params, self._offs)):
                return cand
        return None

    @torch.no_grad()
    def step(self, closure=None):
        g = self._flat_grad()
        grp = self.param_groups[0]
        if g is None or len(self.param_groups) != 1 or grp.get("amsgrad") or grp.get("maximize"):
            out = super().step(closure)              # not our layout: torch's own update on the same state tensors
            if self.ema is not None:                 # ... which has moved the step counters: t = steps[0] as it stands now
                ops.ema_flat(self.ema, self._flat_p, self._steps, self.ema_decay, self.ema_warmup)
            return out
        lr = grp["lr"]
        if not isinstance(lr, torch.Tensor):
            self._lr_dev.fill_(float(lr))
            lr = self._lr_dev
        b1, b2 = grp["betas"]
        if self.ema is not None:
            ops.adam_flat_ema(self._flat_p, g, self._m, self._v, self.ema, lr, self._steps, b1, b2, grp["eps"], grp["weight_decay"],
                              self.ema_decay, self.ema_warmup)
        else:
            ops.adam_flat(self._flat_p, g, self._m, self._v, lr, self._steps, b1, b2, grp["eps"], grp["weight_decay"])
        return None
