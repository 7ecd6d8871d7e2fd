"""What the resize round trip's tests (test_resize_refs.py, test_resize_gpu.py) share: an fp64 restatement of sst_rescale's model
 that starts from the fp32 values the kernel reads (the rows' words, the pixels), and the derived bound.  A plain
helper module; numpy only.

THE BOUND (bound() below), for inputs of magnitude <= xmax; u = 2^-24, the relative rounding error of one fp32 operation.
One axis pass with exact weights w (T taps, S = sum|w|) on values of magnitude <= V that already carry an error <= E gives values of
magnitude <= S V with an error of at most
    S E                   the incoming error, amplified by sum|w|
  + T dw V                the kernel's weights differ from the exact ones by at most dw each (below)
  + T u S V               the chain of T fmaf's, each rounding once a partial sum that S V bounds
The per-mode constants:
  area      S = 1, T <= 5 (n_in <= 4 n_out), dw = u / 2: 1 / (b - a) is rounded once
  bilinear  S = 1, T = 2, dw = u: t = fl(rem / den) is off by at most u / 2 (t < 1), 1 - t rounds once more
  bicubic   S = 1.375 (at t = 1/2: 2 (0.09375 + 0.59375); 1.375^2 = 1.89 for a 2-D resize), T = 4, dw = 43 u.  A coefficient is a
            cubic in Horner form, ((a x + b) x + c) x + d, on x in [0, 2]: the two roundings of the innermost stage (magnitudes <= 1.5
            and 3.75) are multiplied by x^2 <= 4 (<= 18 u after the 2.25..3 range of that stage on [1, 2] is used: (1.5 + 3) 4), the
            two of the middle stage (<= 6 and 3) by x <= 2 (18 u), the two of the last stage (<= 3.1 and 1) by 1 (4.1 u); x itself
            (t + 1, 1 - t, 2 - t from a t that is off by u / 2) is off by at most 1.5 u, and the cubics' slopes are at most 1.35 (2 u).
            18 + 18 + 4.1 + 2 < 43.  A fused multiply-add in place of a multiply and an add only removes roundings.
A 2-D resize is the x pass followed by the y pass.  Then the noise, v' = fmaf(sd, z, v), on values of magnitude <= V with error <= E:
    E                          the incoming error
  + 16 u Z sd_max              filter_refs.bound's noise term: Z = 5.9 bounds |z|; sd_max = sqrt(sigma_n^2 + s_p V)
  + Z dsd                      sd is made from the kernel's v, not the restatement's: dsd = 0 without shot noise, else
                               min(sqrt(s_p E), s_p E / (2 sigma_n))  (|sqrt(a + d) - sqrt(a)| <= sqrt(d) and <= d / (2 sqrt(a)))
  + u (V + Z sd_max)           the rounding of the fmaf itself
giving magnitude <= V + Z sd_max.  The resize back is a 2-D resize on those.  With no resize (0, 0) only the noise step applies, on
E = 0.  Nothing in the bound is measured; DESIGN.md section 24 records what the kernel actually does against it."""
import numpy as np

from filter_refs import Z_MAX, gauss_at

U = 2.0 ** -24
MODES = ("area", "bilinear", "bicubic")
S_ABS = (1.0, 1.0, 1.375)
TAPS = (5, 2, 4)
DW = (0.5 * U, 1.0 * U, 43.0 * U)
A = -0.75


def _cc1(x):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def _cc2(x):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def axis_matrix(mode, n_in, n_out):
    """The one-axis resample n_in -> n_out as an fp64 matrix [n_out, n_in]; mode 0 area, 1 bilinear, 2 bicubic.  The taps are made in
    integer arithmetic, as the kernel makes them; t is the exact ratio rounded to fp64."""
    M = np.zeros((n_out, n_in))
    for i in range(n_out):
        if mode == 0:
            a, b = (i * n_in) // n_out, ((i + 1) * n_in + n_out - 1) // n_out
            M[i, a:b] = 1.0 / (b - a)
            continue
        num, den = (2 * i + 1) * n_in - n_out, 2 * n_out
        f = num // den                                   # Python's floor division
        t = (num - f * den) / den
        if mode == 1:
            if num < 0:
                f, t = 0, 0.0
            M[i, min(f, n_in - 1)] += 1 - t
            M[i, min(f + 1, n_in - 1)] += t
        else:
            for k, c in enumerate((_cc2(t + 1), _cc1(t), _cc1(1 - t), _cc2(2 - t))):
                M[i, min(max(f - 1 + k, 0), n_in - 1)] += c
    return M


def resize(x, size, mode):
    """x [..., h, w] fp64 -> [..., size[0], size[1]]."""
    My, Mx = axis_matrix(mode, x.shape[-2], size[0]), axis_matrix(mode, x.shape[-1], size[1])
    return My @ x @ Mx.T


def unpack(row):
    """One row -> (hi, wi, sigma_n, s_p as the fp32 values the kernel reads, in fp64; k0, k1, m1, m2, gray, the bits above)."""
    row = np.asarray(row, np.int32)
    f = row[2:4].view(np.float32).astype(np.float64)
    k = row[4:6].view(np.uint32)
    m = int(row[6])
    return int(row[0]), int(row[1]), f[0], f[1], int(k[0]), int(k[1]), m & 3, (m >> 2) & 3, (m >> 4) & 1, m >> 5


def size_ok(hi, wi, h, w):
    return (hi == 0 and wi == 0) or (hi > 0 and wi > 0 and 4 * hi >= h and hi <= 2 * h and 4 * wi >= w and wi <= 2 * w)


def is_bad(row, h, w):
    hi, wi, sn, sp, _, _, m1, m2, _, high = unpack(row)
    return not size_ok(hi, wi, h, w) or m1 == 3 or m2 == 3 or high != 0 or not sn >= 0 or not sp >= 0


def is_passed(row):
    hi, wi, sn, sp = unpack(row)[:4]
    return hi == 0 and wi == 0 and sn == 0 and sp == 0


def noise_at(v, sn, sp, gray, k0, k1):
    """v [C, H, W] fp64 -> v + sd z: sst_filter2d's noise rule at v's own resolution."""
    C, H, W = v.shape
    pix = np.arange(H * W, dtype=np.uint64).reshape(1, H, W)
    e = np.broadcast_to(pix, (C, H, W)) if gray else pix + np.arange(C, dtype=np.uint64).reshape(C, 1, 1) * np.uint64(H * W)
    sd = sn if sp == 0 else np.sqrt(sp * np.maximum(v, 0.0) + sn * sn)
    return v + sd * gauss_at(e, k0, k1)


def rescale_reference(x, rows, quantise=True):
    """x [B,3,h,w] (the fp32 values), rows int32 [B,8] -> y fp64 [B,3,h,w]."""
    x = np.asarray(x, np.float64)
    rows = np.asarray(rows, np.int32).reshape(-1, 8)
    B, C, h, w = x.shape
    out = np.empty_like(x)
    for b in range(B):
        hi, wi, sn, sp, k0, k1, m1, m2, gray, _ = unpack(rows[b])
        if is_bad(rows[b], h, w):
            out[b] = np.nan
            continue
        if is_passed(rows[b]):
            out[b] = x[b]
            continue
        v = resize(x[b], (hi, wi), m1) if hi else x[b].copy()
        if sn != 0 or sp != 0:
            v = noise_at(v, sn, sp, gray, k0, k1)
        if hi:
            v = resize(v, (h, w), m2)
        if quantise:
            v = np.rint(255.0 * np.clip(v, 0.0, 1.0)) / 255.0
        out[b] = v
    return out


def _resize_step(V, E, mode):
    for _ in range(2):                                   # the x pass, then the y pass
        S, T, dw = S_ABS[mode], TAPS[mode], DW[mode]
        V, E = S * V, S * E + T * dw * V + T * U * S * V
    return V, E


def _noise_step(V, E, sn, sp):
    if sn == 0 and sp == 0:
        return V, E
    sd_max = np.sqrt(sn * sn + sp * V)
    dsd = 0.0
    if sp != 0:
        dsd = np.sqrt(sp * E) if sn == 0 else min(np.sqrt(sp * E), sp * E / (2 * sn))
    return V + Z_MAX * sd_max, E + 16 * U * Z_MAX * sd_max + Z_MAX * dsd + U * (V + Z_MAX * sd_max)


def row_bound(row, xmax=1.0):
    """The most the kernel's unquantised fp32 result of one (legal) row may differ from rescale_reference: the module docstring."""
    hi, wi, sn, sp, _, _, m1, m2, _, _ = unpack(row)
    V, E = float(xmax), 0.0
    if hi:
        V, E = _resize_step(V, E, m1)
    V, E = _noise_step(V, E, sn, sp)
    if hi:
        V, E = _resize_step(V, E, m2)
    return E


def bound(rows, xmax=1.0):
    """[B] per-sample bounds for the rows [B,8]."""
    return np.array([row_bound(r, xmax) for r in np.asarray(rows, np.int32).reshape(-1, 8)])
