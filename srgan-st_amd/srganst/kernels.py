"""The kernel zoo of the second-order degradation: the blur kernels of BSRGAN / Real-ESRGAN as K x K tables
for sst_filter2d's bank.  numpy, fp64.  Every function returns a [K, K] table [dy][dx] (x = columns, y = rows) that sums to 1; the
kernel is drawn on a support x support window (odd, <= K, default K) centred in the table, with zeros around it.

With Sigma = R(theta) diag(s1^2, s2^2) R(theta)^T and q = d^T Sigma^-1 d, d = (dx, dy):
  gaussian              exp(-q / 2)
  generalized_gaussian  exp(-q^beta / 2)
  plateau               1 / (q^beta + 1)
  sinc                  the circular low-pass of cutoff omega: omega J1(omega r) / (2 pi r), omega^2 / (4 pi) at the centre
bank(kernels) stacks tables into the fp32 [M, K, K] array the kernel reads, rounded once."""
from __future__ import annotations

import numpy as np

K_MIN, K_MAX = 3, 21
_J1_POINTS = 512


def bessel_j1(x):
    """J1(x) = (1 / pi) int_0^pi cos(t - x sin t) dt by the midpoint rule with 512 points: the integrand is smooth and periodic,
    so the rule converges geometrically (within 3.5e-16 of scipy.special.j1 on [0, 50])."""
    x = np.asarray(x, np.float64)
    t = (np.arange(_J1_POINTS, dtype=np.float64) + 0.5) * (np.pi / _J1_POINTS)
    return np.cos(t - x[..., None] * np.sin(t)).sum(-1) / _J1_POINTS


def _check_window(K: int, support, who: str) -> int:
    if int(K) != K or not (K_MIN <= K <= K_MAX and K % 2 == 1):
        raise ValueError(f"{who}: K = {K!r} must be odd and in {K_MIN}..{K_MAX}")
    support = K if support is None else support
    if int(support) != support or not (1 <= support <= K and support % 2 == 1):
        raise ValueError(f"{who}: support = {support!r} must be odd and in 1..{K}")
    return int(support)


def _embed(win: np.ndarray, K: int, who: str) -> np.ndarray:
    """The window normalised to sum 1, centred in a K x K table of zeros."""
    s = win.sum()
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"{who}: the kernel's sum {s!r} is not finite and positive")
    out = np.zeros((K, K), np.float64)
    o = (K - win.shape[0]) // 2
    out[o:o + win.shape[0], o:o + win.shape[1]] = win / s
    return out


def _quadratic(support: int, s1: float, s2: float, theta: float, who: str) -> np.ndarray:
    """q = d^T Sigma^-1 d on the support x support window."""
    if not (s1 > 0 and s2 > 0 and np.isfinite(s1) and np.isfinite(s2) and np.isfinite(theta)):
        raise ValueError(f"{who}: the standard deviations ({s1!r}, {s2!r}) must be positive and finite, theta {theta!r} finite")
    d = np.arange(-(support // 2), support // 2 + 1, dtype=np.float64)
    dy, dx = d[:, None], d[None, :]
    c, s = np.cos(theta), np.sin(theta)
    i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    return (c * c * i1 + s * s * i2) * dx * dx + 2.0 * c * s * (i1 - i2) * dx * dy + (s * s * i1 + c * c * i2) * dy * dy


def gaussian(K: int, s1: float, s2: float, theta: float = 0.0, support=None) -> np.ndarray:
    support = _check_window(K, support, "gaussian")
    return _embed(np.exp(-0.5 * _quadratic(support, s1, s2, theta, "gaussian")), K, "gaussian")


def generalized_gaussian(K: int, s1: float, s2: float, theta: float = 0.0, beta: float = 1.0, support=None) -> np.ndarray:
    support = _check_window(K, support, "generalized_gaussian")
    if not (beta > 0 and np.isfinite(beta)):
        raise ValueError(f"generalized_gaussian: beta = {beta!r} must be positive and finite")
    return _embed(np.exp(-0.5 * _quadratic(support, s1, s2, theta, "generalized_gaussian") ** beta), K, "generalized_gaussian")


def plateau(K: int, s1: float, s2: float, theta: float = 0.0, beta: float = 1.0, support=None) -> np.ndarray:
    support = _check_window(K, support, "plateau")
    if not (beta > 0 and np.isfinite(beta)):
        raise ValueError(f"plateau: beta = {beta!r} must be positive and finite")
    return _embed(1.0 / (_quadratic(support, s1, s2, theta, "plateau") ** beta + 1.0), K, "plateau")


def sinc(K: int, omega: float, support=None) -> np.ndarray:
    """The circular (2-D ideal) low-pass filter of cutoff omega radians per pixel, 0 < omega <= pi, truncated to the window."""
    support = _check_window(K, support, "sinc")
    if not 0 < omega <= np.pi:
        raise ValueError(f"sinc: omega = {omega!r} must be in (0, pi]")
    d = np.arange(-(support // 2), support // 2 + 1, dtype=np.float64)
    r = np.hypot(d[:, None], d[None, :])
    centre = r == 0
    rs = np.where(centre, 1.0, r)
    win = np.where(centre, omega * omega / (4.0 * np.pi), omega * bessel_j1(omega * rs) / (2.0 * np.pi * rs))
    return _embed(win, K, "sinc")


def bank(kernels) -> np.ndarray:
    """[M, K, K] fp32, C-contiguous, from M tables of one size K: each normalised in fp64 (a table whose sum is not finite and
    positive is refused), then rounded once.  An empty list gives [0, 0, 0]."""
    ks = [np.asarray(k, np.float64) for k in kernels]
    if not ks:
        return np.zeros((0, 0, 0), np.float32)
    K = ks[0].shape[0]
    out = np.empty((len(ks), K, K), np.float32)
    for m, k in enumerate(ks):
        if k.shape != (K, K) or not (K_MIN <= K <= K_MAX and K % 2 == 1):
            raise ValueError(f"bank: kernel {m} is {k.shape}; every kernel must be K x K with one odd K in {K_MIN}..{K_MAX}")
        s = k.sum()
        if not (np.isfinite(k).all() and s > 0):
            raise ValueError(f"bank: kernel {m}'s sum {s!r} is not finite and positive")
        out[m] = (k / s).astype(np.float32)
    return out
