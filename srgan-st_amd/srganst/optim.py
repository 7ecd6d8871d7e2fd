"""Adam on flat buffers: torch.optim.Adam's interface and state layout, one HIP kernel per step.

The reference builds ``optim.Adam(params, lr, betas, eps, weight_decay)`` (train.py:62-75, warmup.py:34-40) and steps LR
schedulers on it.  FlatAdam IS a torch.optim.Adam (schedulers, ``param_groups``, ``state_dict()`` / ``load_state_dict()``
keep working and checkpoints stay interchangeable); what changes is where the numbers live: parameters, gradients and
both moments are flat fp32 buffers of one layout, so ``step()`` is a single streaming pass (csrc/optim.hip) instead of
torch's multi-tensor launches (measured 130 us -> ~12 us per generator step on MI355X).

With ``ema_decay > 0`` the same pass also keeps an exponential moving average of the parameters in a flat buffer of the
parameters' layout (``ema``): ema <- d * ema + (1 - d) * p_new, d = ema_decay or, with ``ema_warmup``,
min(ema_decay, (1 + t) / (10 + t)) at Adam step t.  The average is NOT part of ``state_dict()`` (that stays torch's
layout); it travels as the state dict of a module whose parameters are views of the buffer (engine: ``g_ema``).

``max_grad_norm > 0`` clips the gradient to that global L2 norm (``torch.nn.utils.clip_grad_norm_``'s rule) and
``skip_nonfinite`` drops an update whose gradient holds a NaN or an infinity - weights, moments, step counters and the average
stay as they were.  Both decisions are taken on the device (one fp64 reduction over the parameter elements of the flat
gradient, ``ops.grad_sumsq``, then ``ops.adam_flat_clip``), so they ride in a captured graph with no host sync.  The outcome
is ``grad_record`` (device) / ``grad_stats()`` (host); the cumulative counters travel with the training state
(``clip_counters`` / ``load_clip_counters``), not in ``state_dict()``.  With both off ``step()`` is the code it always was."""
from __future__ import annotations

import math

import torch

from . import _abi, ops
from ._state import state

NORM_CHUNK = 8192            # floats per job of the norm reduction: one workgroup of 256 lanes, eight float4 loads each
RECORD_FIELDS = ("norm", "coef", "skipped_now", "n_skipped", "n_clipped", "n_steps_seen")
COUNTER_FIELDS = RECORD_FIELDS[3:]


def norm_jobs(offsets, numels, chunk=NORM_CHUNK):
    """The job table of the norm reduction: [(start, count)] covering every parameter element of a flat buffer exactly once and
    no pad word, count <= chunk.  Pure Python."""
    if chunk <= 0:
        raise ValueError(f"chunk must be positive, got {chunk}")
    jobs = []
    for o, n in zip(offsets, numels):
        for s in range(0, int(n), int(chunk)):
            jobs.append((int(o) + s, min(int(chunk), int(n) - s)))
    return jobs


class FlatAdam(torch.optim.Adam):
    def __init__(self, module, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, ema_decay=0.0,
                 ema_warmup=True, ema_buffer=None, max_grad_norm=0.0, skip_nonfinite=False):
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        if not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0 (0 = no clipping), got {max_grad_norm}")
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
        # clipping / the guard: job table, partials and the record exist before any graph capture too
        self.max_grad_norm, self.skip_nonfinite = float(max_grad_norm), bool(skip_nonfinite)
        self.clip_on = self.max_grad_norm > 0.0 or self.skip_nonfinite
        self.grad_record = self._jobs = self._partials = None
        if self.clip_on:
            self.grad_record = torch.zeros(len(RECORD_FIELDS), device=dev, dtype=torch.float64)
            if dev.type == "cuda":
                self._jobs = ops.NormJobs(norm_jobs(offs, [p.numel() for p in params]), dev)
                self._partials = torch.zeros(self._jobs.njobs, device=dev, dtype=torch.float64)

    def grad_stats(self):
        """The record of the last step as Python numbers (one host copy, for logging), or None with the feature off."""
        if self.grad_record is None:
            return None
        r = self.grad_record.tolist()
        out = dict(zip(RECORD_FIELDS, r))
        for k in RECORD_FIELDS[2:]:
            out[k] = int(out[k])
        return out

    def clip_counters(self):
        """The cumulative counters, for the training state (checkpoint.py); None with the feature off."""
        st = self.grad_stats()
        return None if st is None else {k: st[k] for k in COUNTER_FIELDS}

    @torch.no_grad()
    def load_clip_counters(self, counters):
        """Counters a training state carried; None (a file without them) leaves them at zero."""
        if self.grad_record is None or not counters:
            return
        self.grad_record[3:] = torch.tensor([float(counters.get(k, 0)) for k in COUNTER_FIELDS], dtype=torch.float64)

    def _stock_clip(self):
        """Clipping and the guard for the stock-torch update (gradients that are not the flat views), with torch ops; eager only
        (the finiteness test reads a value on the host).  Returns True when the step is to be skipped."""
        if torch.cuda.is_current_stream_capturing():
            raise _abi.HipPathError("FlatAdam: max_grad_norm / skip_nonfinite on gradients that are not the flat_grads views need a "
                                    "host decision and cannot be captured into a graph")
        params = [p for p in self._params if p.grad is not None]
        norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in params])))
        skip = self.skip_nonfinite and not math.isfinite(norm)
        coef = 1.0
        if not skip and self.max_grad_norm > 0.0:
            total = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm, foreach=True)
            coef = float(torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0))
        st = self.grad_stats()
        rec = [norm, coef, float(skip), st["n_skipped"] + int(skip), st["n_clipped"] + int(not skip and coef < 1.0),
               st["n_steps_seen"] + 1]
        self.grad_record.copy_(torch.tensor(rec, dtype=torch.float64))
        return skip

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
            if self.clip_on and self._stock_clip():
                return None
            out = super().step(closure)              # not our layout: torch's own update on the same state tensors
            if self.ema is not None:                 # ... which has moved the step counters: t = steps[0] as it stands now
                ops.ema_flat(self.ema, self._flat_p, self._steps, self.ema_decay, self.ema_warmup)
            return out
        lr = grp["lr"]
        if not isinstance(lr, torch.Tensor):
            self._lr_dev.fill_(float(lr))
            lr = self._lr_dev
        b1, b2 = grp["betas"]
        if self.clip_on:
            ops.grad_sumsq(g, self._jobs, self._partials)
            ops.adam_flat_clip(self._flat_p, g, self._m, self._v, self.ema, lr, self._steps, b1, b2, grp["eps"], grp["weight_decay"],
                               self.ema_decay, self.ema_warmup, self._partials, self._jobs.njobs, self.max_grad_norm,
                               self.skip_nonfinite, self.grad_record)
        elif self.ema is not None:
            ops.adam_flat_ema(self._flat_p, g, self._m, self._v, self.ema, lr, self._steps, b1, b2, grp["eps"], grp["weight_decay"],
                              self.ema_decay, self.ema_warmup)
        else:
            ops.adam_flat(self._flat_p, g, self._m, self._v, lr, self._steps, b1, b2, grp["eps"], grp["weight_decay"])
        return None
