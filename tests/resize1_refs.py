"""What the tests of the first stage's random resize (test_resize1_refs.py, test_resize1_gpu.py) share: an fp64 restatement of
sst_rescale_to's model that starts from the fp32 values the kernel reads (the rows' words, the pixels), and the
derived bound.  The one-axis matrices, the rows' layout and the noise rule are resize_refs' (section 24): the chain is the same, only
the output geometry is the launch's own.  A plain helper module; numpy only.

THE BOUND (bound() below), for inputs of magnitude <= xmax; u = 2^-24.  Section 24's formula, unchanged: one axis pass with exact
weights w (T taps, S = sum|w|) on values of magnitude <= V that carry an error <= E gives magnitude <= S V and an error of at most
    S E + T dw V + T u S V
with dw the most a kernel weight differs from the exact one: area u / 2 (1 / (b - a) is rounded once), bilinear u, bicubic 43 u
(resize_refs' docstring has the arithmetic), and S = 1, 1, 1.375.  What changes is T.  Section 24 could take area's T <= 5 from its
ratio cap; here the tap counts are the ACTUAL ones of each of the four passes, max_i (b_i - a_i) of that axis:
    x pass W -> wi and y pass H -> hi with m1:  area at most ceil(W / wi) + 1 <= 9 taps (8 wi >= W); bilinear 2; bicubic 4
    noise at (hi, wi): section 24's term,  E + 16 u Z sd_max + Z dsd + u (V + Z sd_max),  magnitude V + Z sd_max
    x pass wi -> w and y pass hi -> h with m2:  area at most ceil(wi / w) + 1 <= 2 W / w + 1 taps (33 at W = 16 w)
A "keep" row (0, 0) has no first resize: E = 0 enters the noise step (the intermediate is the input itself), and the second resize
runs from (H, W).  Worked through for 96 x 96 -> 24 x 24 and inputs in [0, 1]: area to 12 (8 taps) and area down (1 tap) is
2 (8 u / 2 + 8 u) + 2 (u / 2 + u) = 27 u = 1.6e-6; bicubic to 144 and area down (6 taps) 3.1e-5, of which the bicubic passes are
the x pass's 4 (43 u + 1.375 u) = 177.5 u and the y pass's 1.375 (177.5 u) + 1.375 (177.5 u) = 488 u = 2.9e-5 (V grows to 1.375,
then 1.89); bicubic both ways at 48 1.1e-4; keep with
area down (4 taps) 7.2e-7; keep with noise 20 and bicubic down 4.4e-5; shot noise alone (s_p = 0.02) behind a bicubic resize 4.5e-3 -
section 24's loose case, sqrt(s_p E) with no Gaussian floor.  Nothing in the bound is measured; DESIGN.md section 25 records what
the kernel does against it."""
import numpy as np

import resize_refs as r24
from resize_refs import MODES, U, axis_matrix, noise_at, resize, unpack  # noqa: F401  (re-exported for the tests)

MIN_DIV, MAX_RATIO, MAX_DOWN = 8, 2, 16


def size_ok(hi, wi, H, W):
    return (hi == 0 and wi == 0) or (hi > 0 and wi > 0 and MIN_DIV * hi >= H and hi <= MAX_RATIO * H and MIN_DIV * wi >= W
                                     and wi <= MAX_RATIO * W)


def is_bad(row, H, W):
    hi, wi, sn, sp, _, _, m1, m2, _, high = unpack(row)
    return not size_ok(hi, wi, H, W) or m1 == 3 or m2 == 3 or high != 0 or not sn >= 0 or not sp >= 0


def taps(mode, n_in, n_out):
    """The largest tap count of the one-axis resample n_in -> n_out."""
    if mode == 0:
        return max(((i + 1) * n_in + n_out - 1) // n_out - (i * n_in) // n_out for i in range(n_out))
    return (2, 4)[mode - 1]


def rescale_to_reference(x, rows, size, quantise=True):
    """x [B,3,H,W] (the fp32 values), rows int32 [B,8], size (h, w) -> y fp64 [B,3,h,w]."""
    x = np.asarray(x, np.float64)
    rows = np.asarray(rows, np.int32).reshape(-1, 8)
    B, C, H, W = x.shape
    h, w = size
    out = np.empty((B, C, h, w))
    for b in range(B):
        hi, wi, sn, sp, k0, k1, m1, m2, gray, _ = unpack(rows[b])
        if is_bad(rows[b], H, W):
            out[b] = np.nan
            continue
        if (H, W) == (h, w) and r24.is_passed(rows[b]):
            out[b] = x[b]
            continue
        v = resize(x[b], (hi, wi), m1) if hi else x[b].copy()
        if sn != 0 or sp != 0:
            v = noise_at(v, sn, sp, gray, k0, k1)
        if hi or (H, W) != (h, w):
            v = resize(v, (h, w), m2)
        if quantise:
            v = np.rint(255.0 * np.clip(v, 0.0, 1.0)) / 255.0
        out[b] = v
    return out


def _axis_step(V, E, mode, n_in, n_out):
    S, T, dw = r24.S_ABS[mode], taps(mode, n_in, n_out), r24.DW[mode]
    return S * V, S * E + T * dw * V + T * U * S * V


def row_bound(row, H, W, h, w, xmax=1.0):
    """The most the kernel's unquantised fp32 result of one (legal) row may differ from rescale_to_reference: the module docstring."""
    hi, wi, sn, sp, _, _, m1, m2, _, _ = unpack(row)
    V, E = float(xmax), 0.0
    if hi:
        V, E = _axis_step(V, E, m1, W, wi)
        V, E = _axis_step(V, E, m1, H, hi)
    else:
        hi, wi = H, W
    V, E = r24._noise_step(V, E, sn, sp)
    if (hi, wi) != (H, W) or (H, W) != (h, w) or unpack(row)[0]:
        V, E = _axis_step(V, E, m2, wi, w)
        V, E = _axis_step(V, E, m2, hi, h)
    return E


def bound(rows, H, W, h, w, xmax=1.0):
    """[B] per-sample bounds for the rows [B,8]."""
    return np.array([row_bound(r, H, W, h, w, xmax) for r in np.asarray(rows, np.int32).reshape(-1, 8)])
