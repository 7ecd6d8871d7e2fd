"""What the HIP path keeps per nn.Module: its caches, and the protocol between a step engine and the discriminator's graph.

``state(module)`` is the module's HipState, created on first use.  It sits under ONE key of ``module.__dict__`` - not a
parameter, buffer or submodule - so it never enters state_dict(), named_buffers() or parameters().  Nothing outside this file
touches ``module.__dict__``.
"""
from __future__ import annotations

from contextlib import contextmanager

_KEY = "_hip_state"


class GradScope:
    """One accumulation scope (HipState.accumulating_grads): `flat` is the flat gradient buffer its first backward pass wrote,
    None until then."""

    def __init__(self):
        self.flat = None


class KeptPass:
    """A discriminator pass kept for re-use by the step engine (HipState.keep_pass): the identity of its input, its logits, the
    tensors its backward reads, the detached parameters it ran on and the PassArena it wrote into (or None)."""

    def __init__(self, x_ptr, x_shape, out, sv, p, arena):
        self.x_ptr, self.x_shape, self.out, self.sv, self.p, self.arena = x_ptr, x_shape, out, sv, p, arena
        # as numbers: a detached parameter shares its version counter with the live one, so p[n]._version moves along with it
        self.versions = {n: t._version for n, t in p.items()}

    def is_pass_over(self, x, pd, names):
        """Is this a pass over `x` with the weights `pd` as they are now (none rebound, none modified through torch)?"""
        return (self.x_ptr == x.data_ptr() and self.x_shape == tuple(x.shape)
                and all(self.p[n].data_ptr() == pd[n].data_ptr() and self.versions[n] == pd[n]._version for n in names))


class HipState:
    def __init__(self):
        # ---- caches, for any module
        self.cache = {}             # packed weights and their launch plans (ops.packed_weights), by key
        self.flat_params = None     # (flat, offsets) once ops.flatten_params has moved the parameters into one buffer
        # ops.flat_grads: a ring of ops.FLAT_RING persistent, zero-initialised flat gradient buffers
        # {"total", "device", "next", "bufs"}, allocated at the first call (always an eager warm-up call: never inside a graph
        # capture) and handed out in turn.  The pad words between the views (ops.flat_layout) are written by nobody, so they stay
        # zero for good - they travel through the flat Adam and the all-reduce with the real gradients, and an uninitialised NaN
        # there would poison any norm / isfinite check over the flat buffer.  A buffer comes round again after FLAT_RING - 1 other
        # backward passes of the module (at most two per step are alive at once: the two-stream discriminator step).
        self.flat_ring = None
        # the ring's buffers in order of use, the last four: with two backward passes per step (D on gt and on sr) autograd
        # accumulates into the FIRST pass's buffer, which is then the one holding p.grad (dist.module_flat_grad finds it)
        self.flat_grads = []
        self.nbt_flat = None        # the int64 tensor every BatchNorm's num_batches_tracked is a view of (ops.flatten_bn_counters)
        self.bn_acc_buf = None      # generator, accumulator mode: the fp64 statistics accumulators of forward and backward, one buffer
        self.bn_acc_token = None    # ... identity of the forward that cleared them last; None once a backward has dirtied its half

        # ---- owner protocol of the discriminator
        # The discriminator runs up to three forward and three backward passes between two updates of its weights (train.py:125-161:
        # D(sr) in the generator step, D(gt) and D(sr) in its own step).  An owner controls those updates (engine.TrainEngine: D's
        # packed weights are made once per iteration, by the D(sr) of the generator step, and re-used by the passes of the
        # discriminator step) and clears packs_fresh after every optimizer step; while there is an owner and the packs are fresh
        # (and no parameter was rebound or modified through torch, see _version) disc_graph.packs hands the packed buffers out again
        # without a launch.  Without an owner every call packs.
        self.owner = None
        self.packs_fresh = False
        self.keep_pass = False      # a training pass with grad leaves itself in last_pass (set by keeping_pass only)
        self.arena_request = None   # (slots, slot): the kept pass writes into that slot of a fresh disc_graph.PassArena
        self.last_pass = None       # KeptPass: the generator step's D(sr), which the discriminator step re-uses instead of running it again
        self.counters_external = False      # the owner adds the passes of an iteration to the BatchNorm batch counters itself
        # Two backward passes per D step (D(gt) and D(sr), train.py:155-161): inside a GradScope the second pass ADDS into the first
        # pass's flat buffer with the kernels' accumulate flag and hands autograd nothing - p.grad stays a view of ONE flat buffer
        # (flat Adam, single RCCL message) and autograd's own out-of-place sum of two 94 MB gradient sets disappears.
        self.grad_accum = None

    # ---- the scoped fields: set for the body, restored however it ends
    @contextmanager
    def keeping_pass(self, arena_request=None):
        self.keep_pass, self.arena_request, self.last_pass = True, arena_request, None
        try:
            yield
        finally:
            self.keep_pass, self.arena_request = False, None      # last_pass stays: the discriminator step reads it

    @contextmanager
    def external_counters(self):
        self.counters_external = True
        try:
            yield
        finally:
            self.counters_external = False

    @contextmanager
    def accumulating_grads(self):
        scope = self.grad_accum = GradScope()
        try:
            yield scope
        finally:
            self.grad_accum = None


def state(module) -> HipState:
    st = module.__dict__.get(_KEY)
    if st is None:
        st = module.__dict__[_KEY] = HipState()
    return st
