"""What the second-order degradation tests (test_filter_refs.py, test_filter_gpu.py) share: an fp64 restatement of sst_filter2d's
model that starts from the fp32 values the kernel reads (the rows' words, the bank), the derived bound, and the
fixed bank and rows of the GPU cases.  A plain helper module; numpy only."""
import numpy as np

from degrade_refs import philox4x32

Z_MAX = 5.9         # Box-Muller on u1 >= 2^-25: |z| <= sqrt(2 * 25 * ln 2) = 5.887


def unpack(row):
    """One row -> (idx, sigma_n, s_p as the fp32 values the kernel reads, in fp64; gray, k0, k1)."""
    row = np.asarray(row, np.int32)
    f = row[1:3].view(np.float32).astype(np.float64)
    k = row[4:6].view(np.uint32)
    return int(row[0]), f[0], f[1], int(row[3]), int(k[0]), int(k[1])


def gauss_at(e, k0, k1):
    """The standard normals of the elements e (any shape), in fp64: Philox4x32-10 at counter (e, 0, 0, 0), Box-Muller."""
    e = np.asarray(e, np.uint64)
    x = philox4x32([e, np.zeros_like(e), np.zeros_like(e), np.zeros_like(e)], (k0, k1))
    u1 = ((x[0] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((x[1] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def correlate(x, k):
    """x [C,h,w], k [K,K] fp64 -> sum_{dy,dx} k[dy][dx] x[refl(y+dy-p)][refl(x+dx-p)]: a correlation under torch's `reflect`."""
    K = k.shape[0]
    p = K // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p)), mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, (K, K), axis=(1, 2))      # [C, h, w, K, K]
    return np.einsum("chwij,ij->chw", win, k)


def is_passed(row):
    idx, sn, sp, _, _, _ = unpack(row)
    return idx == -1 and sn == 0 and sp == 0


def is_bad(row, M):
    idx, sn, sp, gray, _, _ = unpack(row)
    return idx < -1 or idx >= M or gray not in (0, 1) or not sn >= 0 or not sp >= 0


def filter_reference(x, flt, bank, quantise=True):
    """x [B,3,h,w] (the fp32 values), flt int32 [B,8], bank fp32 [M,K,K] or None -> y fp64 [B,3,h,w]."""
    x = np.asarray(x, np.float64)
    flt = np.asarray(flt, np.int32).reshape(-1, 8)
    M = 0 if bank is None else len(bank)
    B, C, h, w = x.shape
    out = np.empty_like(x)
    pix = np.arange(h * w, dtype=np.uint64).reshape(1, h, w)
    for b in range(B):
        idx, sn, sp, gray, k0, k1 = unpack(flt[b])
        if is_bad(flt[b], M):
            out[b] = np.nan
            continue
        if is_passed(flt[b]):
            out[b] = x[b]
            continue
        v = correlate(x[b], np.asarray(bank[idx], np.float64)) if idx >= 0 else x[b].copy()
        if sn != 0 or sp != 0:
            e = np.broadcast_to(pix, (C, h, w)) if gray else pix + np.arange(C, dtype=np.uint64).reshape(C, 1, 1) * np.uint64(h * w)
            sd = sn if sp == 0 else np.sqrt(sp * np.maximum(v, 0.0) + sn * sn)
            v = v + sd * gauss_at(e, k0, k1)
        if quantise:
            v = np.rint(255.0 * np.clip(v, 0.0, 1.0)) / 255.0
        out[b] = v
    return out


def bound(K, bank, flt=None, xmax=1.0):
    """The most the kernel's unquantised fp32 result may differ from filter_reference, for inputs in [0, xmax] - derived, not measured:
      blur   (K^2 + 6) 2^-24 max_m sum|bank[m]| max|x|: a chain of K^2 fmaf's, each rounding once a partial sum that sum|w| max|x|
             bounds, and the roundings around it (without a bank: the identity, sum|w| = 1)
      noise  16 2^-24 * 5.9 * sd_max, sd_max = sqrt(sigma_n^2 + s_p), taken at v = 1, over the rows flt: 5.9 bounds |z|, 16 ulps is twice
             the sum of the documented errors of logf, sqrtf, cospif and the two roundings."""
    sabs = 1.0 if bank is None or not len(bank) else float(np.abs(np.asarray(bank, np.float64)).sum((1, 2)).max())
    blur = (K * K + 6) * 2.0 ** -24 * sabs * xmax
    noise = 0.0
    if flt is not None:
        for row in np.asarray(flt, np.int32).reshape(-1, 8):
            _, sn, sp, _, _, _ = unpack(row)
            if np.isfinite(sn) and np.isfinite(sp) and sn >= 0 and sp >= 0:
                noise = max(noise, 16 * 2.0 ** -24 * Z_MAX * np.sqrt(sn * sn + sp))
    return blur + noise


def one_hot(K, dy, dx):
    k = np.zeros((K, K))
    k[dy, dx] = 1.0
    return k


def shifted(x, K, dy, dx):
    """What the one-hot kernel at [dy][dx] makes of x [..., h, w]: out[y][x] = X[refl(y + dy - p)][refl(x + dx - p)], exactly."""
    p = K // 2
    h, w = x.shape[-2:]
    refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    iy, ix = refl(np.arange(h) + dy - p, h), refl(np.arange(w) + dx - p, w)
    return x[..., iy[:, None], ix[None, :]]


def case_bank(K):
    """The GPU cases' bank for a window K, fp32 [M,K,K], and the names of its kernels: an anisotropic Gaussian, a generalised Gaussian,
    a plateau, sinc at pi/3 and at pi, a kernel on a smaller support inside K (7 inside 21), and a one-hot off-centre kernel."""
    from srganst import kernels
    small = 7 if K > 7 else max(1, K - 2)
    tables = [
        ("aniso", kernels.gaussian(K, 0.7 + K / 10, 0.4 + K / 30, 0.6)),
        ("generalized", kernels.generalized_gaussian(K, 1.2, 0.8, 2.1, beta=0.7)),
        ("plateau", kernels.plateau(K, 1.5, 1.0, 1.0, beta=1.6)),
        ("sinc_pi3", kernels.sinc(K, np.pi / 3)),
        ("sinc_pi", kernels.sinc(K, np.pi)),
        ("support", kernels.plateau(K, 1.1, 1.9, 0.3, beta=1.2, support=small)),
        ("one_hot", one_hot(K, *one_hot_at(K))),
    ]
    return kernels.bank([t for _, t in tables]), [n for n, _ in tables]


def one_hot_at(K):
    """(dy, dx) of the one-hot kernel: off centre, different in the two axes, in the window's corner region."""
    return (0, K - 2)
