"""CPU: the host side of the second-order degradation - the kernel zoo of srganst.kernels, the fp64 restatement
of sst_filter2d in tests/filter_refs.py, the rows and draws of srganst.device_data (filter_rows, SecondOrder, DeviceCropLoader) and the
config switches."""
import numpy as np
import pytest
import torch

import degrade_refs
import filter_refs as refs
from test_degrade_refs import _Arena

PI = np.pi


def _k():
    from srganst import kernels
    return kernels


# ---- bessel_j1
def test_bessel_j1_known_values():
    k = _k()
    assert abs(float(k.bessel_j1(1.0)) - 0.4400505857449335) < 1e-15
    assert abs(float(k.bessel_j1(10.0)) - 0.04347274616886144) < 1e-15
    assert abs(float(k.bessel_j1(3.8317059702075125))) < 1e-15
    assert float(k.bessel_j1(0.0)) == 0.0 or abs(float(k.bessel_j1(0.0))) < 1e-16
    x = np.linspace(0.0, 50.0, 7)
    assert k.bessel_j1(x).shape == (7,) and k.bessel_j1(x.reshape(7, 1)).shape == (7, 1)
    assert np.allclose(k.bessel_j1(-x), -k.bessel_j1(x), atol=1e-15)                 # odd


def test_bessel_j1_against_scipy():
    special = pytest.importorskip("scipy.special")
    x = np.linspace(0.0, 50.0, 20001)
    err = np.abs(_k().bessel_j1(x) - special.j1(x)).max()
    print(f"bessel_j1 against scipy.special.j1 on [0, 50]: {err:.3g}")
    assert err <= 3.5e-16


# ---- the families
def _quadratic_weights(K, s1, s2, theta):
    """degrade_rows' parameters (A/2, B, C/2) in fp64, before their rounding to fp32, through degrade_refs.weights."""
    i1, i2 = 1.0 / s1 ** 2, 1.0 / s2 ** 2
    c, s = np.cos(theta), np.sin(theta)
    return degrade_refs.weights(0.5 * (c * c * i1 + s * s * i2), c * s * (i1 - i2), 0.5 * (s * s * i1 + c * c * i2), K)


@pytest.mark.parametrize("K", [3, 7, 21])
def test_gaussian_is_the_first_stage_kernel(K):
    from srganst.device_data import degrade_rows
    k = _k()
    for s1, s2, theta in ((0.7, 2.9, 0.4), (4.0, 0.2, 2.5), (1.3, 1.3, 0.0), (2.0, 0.9, PI / 2)):
        assert np.abs(k.gaussian(K, s1, s2, theta) - _quadratic_weights(K, s1, s2, theta)).max() <= 1e-14
    # through degrade_rows itself where its fp32 words are exact: powers of two at theta = 0
    for s1, s2 in ((1.0, 2.0), (0.5, 4.0), (2.0, 2.0)):
        qa, qb, qc, _, _, _ = degrade_refs.unpack(degrade_rows([s1], [s2], [0.0], [0.0], [(0, 0)])[0])
        assert np.abs(k.gaussian(K, s1, s2, 0.0) - degrade_refs.weights(qa, qb, qc, K)).max() <= 1e-14


def test_generalized_gaussian_and_plateau():
    k = _k()
    for K, s1, s2, theta in ((7, 0.8, 1.7, 0.3), (21, 2.5, 1.1, 2.0)):
        assert np.array_equal(k.generalized_gaussian(K, s1, s2, theta, beta=1.0), k.gaussian(K, s1, s2, theta))
        assert not np.array_equal(k.generalized_gaussian(K, s1, s2, theta, beta=0.5), k.gaussian(K, s1, s2, theta))
    # plateau at hand-computed points: isotropic s = 2, beta = 2: q = r^2 / 4, w = 1 / (q^2 + 1) -> centre 1, (0,2): q = 1 -> 1/2,
    # (2,2): q = 2 -> 1/5, (0,1): q = 1/4 -> 16/17
    t = k.plateau(5, 2.0, 2.0, 0.0, beta=2.0)
    c = t[2, 2]
    assert abs(t[2, 4] / c - 0.5) < 1e-15 and abs(t[4, 4] / c - 0.2) < 1e-15 and abs(t[2, 3] / c - 16.0 / 17.0) < 1e-15
    # anisotropic, theta = 0: s1 along x = columns.  s1 = 1, s2 = 2, beta = 1: (dy 0, dx 1): q = 1 -> 1/2; (dy 1, dx 0): q = 1/4 -> 4/5
    t = k.plateau(3, 1.0, 2.0, 0.0, beta=1.0)
    assert abs(t[1, 2] / t[1, 1] - 0.5) < 1e-15 and abs(t[2, 1] / t[1, 1] - 0.8) < 1e-15
    # theta = pi / 2 turns the first axis onto y = rows
    t = k.plateau(3, 1.0, 2.0, PI / 2, beta=1.0)
    assert abs(t[2, 1] / t[1, 1] - 0.5) < 1e-15 and abs(t[1, 2] / t[1, 1] - 0.8) < 1e-15
    # generalised Gaussian at a hand-computed point: isotropic s = 1, beta = 2, (0, 1): q = 1 -> exp(-1/2); (1, 1): q = 2 -> exp(-2)
    t = k.generalized_gaussian(3, 1.0, 1.0, 0.0, beta=2.0)
    assert abs(t[1, 2] / t[1, 1] - np.exp(-0.5)) < 1e-15 and abs(t[2, 2] / t[1, 1] - np.exp(-2.0)) < 1e-15


def _families(K, support=None):
    k = _k()
    return {
        "gaussian": k.gaussian(K, 1.4, 0.6, 0.7, support=support),
        "generalized": k.generalized_gaussian(K, 0.9, 2.2, 2.6, beta=3.1, support=support),
        "plateau": k.plateau(K, 1.5, 0.8, 1.1, beta=1.7, support=support),
        "sinc": k.sinc(K, 1.9, support=support),
        "sinc_pi": k.sinc(K, PI, support=support),
    }


@pytest.mark.parametrize("K, support", [(3, None), (7, None), (7, 3), (21, None), (21, 7), (13, 13), (21, 1)])
def test_every_family_sums_to_one_is_symmetric_and_stays_in_its_support(K, support):
    s = K if support is None else support
    o = (K - s) // 2
    for name, t in _families(K, support).items():
        assert t.shape == (K, K) and t.dtype == np.float64, name
        assert abs(t.sum() - 1.0) <= 1e-15, (name, t.sum() - 1.0)
        assert np.array_equal(t, t[::-1, ::-1]), name                                 # 180 degrees
        inside = np.zeros((K, K), bool)
        inside[o:o + s, o:o + s] = True
        assert (t[~inside] == 0).all() and (t[inside] != 0).any(), name
        assert t[K // 2, K // 2] == t.max(), name


def test_sinc_centre_and_off_centre_values():
    k = _k()
    for K, omega in ((7, 1.0), (21, PI / 3), (13, PI)):
        t = k.sinc(K, omega)
        c = K // 2
        raw_c = omega * omega / (4 * PI)
        for dy, dx in ((0, 1), (2, 3), (c, c)):
            r = np.hypot(dy, dx)
            want = omega * float(k.bessel_j1(omega * r)) / (2 * PI * r)
            assert abs(t[c + dy, c + dx] / t[c, c] - want / raw_c) < 1e-13


@pytest.mark.parametrize("omega", [PI / 3, PI / 2, 2.0])
@pytest.mark.parametrize("K", [7, 13, 21])
def test_sinc_is_a_low_pass(K, omega):
    """|DFT| on 64 x 64: its mean over |f| >= 1.5 omega (within Nyquist in both axes) is below 0.1 x its mean over |f| <= 0.5 omega;
    the DC response is 1."""
    t = _k().sinc(K, omega)
    F = np.abs(np.fft.fft2(t, (64, 64)))
    f = 2 * PI * np.fft.fftfreq(64)
    r = np.hypot(f[:, None], f[None, :])
    stop, keep = F[r >= 1.5 * omega], F[r <= 0.5 * omega]
    ratio = stop.mean() / keep.mean()
    print(f"sinc K = {K}, omega = {omega:.4f}: stop / pass = {ratio:.4f}")
    assert stop.size and keep.size and ratio < 0.1
    assert abs(F[0, 0] - 1.0) < 1e-14


def test_kernel_refusals_and_bank():
    k = _k()
    for fn, args in ((k.gaussian, (4, 1, 1)), (k.gaussian, (23, 1, 1)), (k.gaussian, (1, 1, 1)), (k.plateau, (7, 0.0, 1.0)),
                     (k.gaussian, (7, 1.0, -1.0)), (k.gaussian, (7, float("nan"), 1.0)), (k.sinc, (7, 0.0)), (k.sinc, (7, 3.2)),
                     (k.sinc, (7, -1.0))):
        with pytest.raises(ValueError):
            fn(*args)
    for kw in ({"support": 4}, {"support": 9}, {"support": 0}):
        with pytest.raises(ValueError, match="support"):
            k.gaussian(7, 1.0, 1.0, **kw)
    with pytest.raises(ValueError, match="beta"):
        k.generalized_gaussian(7, 1.0, 1.0, beta=0.0)
    with pytest.raises(ValueError, match="beta"):
        k.plateau(7, 1.0, 1.0, beta=-1.0)
    tables = [k.gaussian(7, 1, 2, 0.3), k.sinc(7, 2.0), 3.0 * refs.one_hot(7, 1, 5)]
    b = k.bank(tables)
    assert b.dtype == np.float32 and b.shape == (3, 7, 7) and b.flags["C_CONTIGUOUS"]
    assert np.array_equal(b[0], tables[0].astype(np.float32)) and np.array_equal(b[2], refs.one_hot(7, 1, 5).astype(np.float32))
    for bad in (np.zeros((7, 7)), -tables[0], np.full((7, 7), np.nan), np.where(refs.one_hot(7, 1, 1) > 0, np.inf, 0.0), tables[1] - 2 * tables[1].mean()):
        with pytest.raises(ValueError, match="not finite and positive"):
            k.bank([tables[0], bad])
    with pytest.raises(ValueError, match="K x K"):
        k.bank([tables[0], k.gaussian(5, 1, 1)])
    with pytest.raises(ValueError, match="K x K"):
        k.bank([np.ones((4, 4))])
    assert k.bank([]).shape == (0, 0, 0)


# ---- the restatement
def test_restatement_against_conv2d():
    """filter_reference's blur against F.pad(reflect) + F.conv2d in fp64; an asymmetric kernel pins the orientation (a correlation)."""
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    for (h, w), K in (((11, 11), 21), ((9, 14), 7), ((2, 2), 3), ((33, 40), 13)):
        p = K // 2
        x = rng.random((2, 3, h, w)).astype(np.float32)
        asym = rng.random((K, K))
        asym[0, K - 1] += 5.0
        bank = np.stack([asym / asym.sum(), refs.one_hot(K, 0, K - 2)]).astype(np.float32)
        rows = np.zeros((2, 8), np.int32)
        rows[:, 0] = (0, 1)
        got = refs.filter_reference(x, rows, bank, quantise=False)
        for b in range(2):
            xp = F.pad(torch.from_numpy(x[b:b + 1]).double(), (p, p, p, p), mode="reflect")
            wgt = torch.from_numpy(bank[b]).double()[None, None].expand(3, 1, K, K)
            want = F.conv2d(xp, wgt, groups=3)[0].numpy()
            assert np.abs(got[b] - want).max() < 1e-14
        assert np.array_equal(got[1], refs.shifted(x[1].astype(np.float64), K, 0, K - 2))
        if min(h, w) > 2:                                # (on 2 x 2 the reflection makes the flipped kernel's sum the same)
            flipped = refs.filter_reference(x[:1], rows[:1], bank[:1, ::-1, ::-1], quantise=False)
            assert np.abs(flipped - got[:1]).max() > 1e-3


def test_restatement_noise_rules():
    from srganst.device_data import filter_rows
    x = np.full((1, 3, 5, 6), 0.5, np.float32)
    x[0, 1] = 0.25
    key = [(123, 456)]
    z = degrade_refs.gauss(90, 123, 456).reshape(3, 5, 6)
    colour = refs.filter_reference(x, filter_rows([-1], 25.5, 0.0, 0, key), None, quantise=False)[0]
    assert np.abs(colour - (x[0] + np.float64(np.float32(0.1)) * z)).max() < 1e-15
    gray = refs.filter_reference(x, filter_rows([-1], 25.5, 0.0, 1, key), None, quantise=False)[0]
    assert np.abs(gray - (x[0] + np.float64(np.float32(0.1)) * z[:1])).max() < 1e-15       # e = y * w + x: channel 0's draws, three times
    sp = np.float64(np.float32(0.02))
    shot = refs.filter_reference(x, filter_rows([-1], 0.0, 0.02, 0, key), None, quantise=False)[0]
    assert np.abs(shot - (x[0] + np.sqrt(sp * x[0].astype(np.float64)) * z)).max() < 1e-15
    both = refs.filter_reference(x - 1.0, filter_rows([-1], 25.5, 0.02, 0, key), None, quantise=False)[0]
    assert np.abs(both - (x[0] - 1.0 + np.float64(np.float32(0.1)) * z)).max() < 1e-15       # v < 0: the shot term is 0
    q = refs.filter_reference(x, filter_rows([-1], 25.5, 0.0, 0, key), None)[0]
    assert np.array_equal(q, np.rint(255 * np.clip(colour, 0, 1)) / 255)
    # pass-through keeps everything; the NaN conventions
    odd = np.array([[np.nan, -3.0, 7.0]], np.float32).reshape(1, 3, 1, 1)
    assert np.array_equal(refs.filter_reference(odd, filter_rows([-1], 0, 0, 0, key), None), odd.astype(np.float64), equal_nan=True)
    bad = filter_rows([-1, 0, -1, -1], 0, 0, 0, key * 4)
    bad[0, 0], bad[1, 0], bad[2, 3], bad[3, 1] = -2, 1, 2, np.float32(-1.0).view(np.int32)
    out = refs.filter_reference(np.zeros((4, 3, 3, 3), np.float32), bad, np.ones((1, 3, 3), np.float32) / 9)
    assert np.isnan(out).all()
    assert refs.bound(21, None) == (441 + 6) * 2.0 ** -24
    b5 = np.stack([np.full((3, 3), 1 / 9), np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float64)]).astype(np.float32)
    assert refs.bound(3, b5) == 15 * 2.0 ** -24 * 9.0
    assert refs.bound(3, None, filter_rows([-1], 25.5, 0.0, 0, key)) == 15 * 2.0 ** -24 + 16 * 2.0 ** -24 * 5.9 * float(np.float32(0.1))


# ---- rows and draws
def test_filter_rows_words_and_refusals():
    from srganst.device_data import filter_rows
    rows = filter_rows([3, -1], [25.5, 0.0], [0.0, 0.0125], [0, 1], [(1, 0xFFFFFFFF), (7, 9)])
    assert rows.dtype == np.int32 and rows.shape == (2, 8)
    assert rows[0].tolist() == [3, int(np.float32(0.1).view(np.int32)), 0, 0, 1, -1, 0, 0]
    assert rows[1].tolist() == [-1, 0, int(np.float32(0.0125).view(np.int32)), 1, 7, 9, 0, 0]
    assert filter_rows([0, 1, 2], 5.0, 0.0, 0, [(0, 0)] * 3).shape == (3, 8)                  # scalars broadcast
    for kw in (dict(noise255=[-1.0]), dict(noise255=[np.nan]), dict(noise255=[np.inf]), dict(shot=[-1e-3]), dict(shot=[np.nan]),
               dict(gray=[2]), dict(gray=[-1]), dict(index=[-2])):
        args = dict(index=[0], noise255=[1.0], shot=[0.0], gray=[0], keys=[(0, 0)])
        args.update(kw)
        with pytest.raises(ValueError, match="filter_rows"):
            filter_rows(**args)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_second_order_draws():
    from srganst.device_data import SecondOrder
    so = SecondOrder()
    n = 20000
    rows = so.draw(n, _gen(3))
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (4, n, 8) and torch.equal(rows, so.draw(n, _gen(3)))
    assert not torch.equal(rows, so.draw(n, _gen(4)))
    a, b, j, c = rows.numpy()
    frac = lambda m: float(np.mean(m))
    # pass A
    assert abs(frac(a[:, 0] >= 0) - 0.8) < 0.02 and a[:, 0].min() == -1 and a[:, 0].max() < 1024 and len(set(a[:, 0].tolist())) > 900
    sn, sp = a[:, 1].copy().view(np.float32) * 255.0, a[:, 2].copy().view(np.float32)
    assert ((sn > 0) ^ (sp > 0)).all()                                            # noise_prob = 1: one of the two, never both
    assert abs(frac(sp > 0) - 0.5) < 0.02 and abs(frac(a[:, 3] == 1) - 0.4) < 0.02 and set(a[:, 3].tolist()) == {0, 1}
    assert sn[sn > 0].min() >= 1.0 - 1e-5 and sn.max() <= 25.0 + 1e-5 and sp[sp > 0].min() >= np.float32(1e-5) and sp.max() <= np.float32(0.025)
    assert (a[:, 6:] == 0).all() and len(set(map(tuple, a[:, 4:6].tolist()))) == n
    # the final sinc: one of B and C, from the bank's sinc section
    sinc = np.maximum(b[:, 0], c[:, 0])
    assert ((b[:, 0] == -1) | (c[:, 0] == -1)).all() and abs(frac(sinc >= 0) - 0.8) < 0.02
    assert sinc[sinc >= 0].min() >= 1024 and sinc.max() < 1280
    assert abs(frac(b[sinc >= 0, 0] >= 0) - 0.5) < 0.02
    for t in (b, c):
        assert (t[:, 1:] == 0).all()                                              # neither noise nor key: pass-through unless sinc
    assert (j[:, :6] == 0).all() and (j[:, 7] == 0).all() and j[:, 6].min() >= 30 and j[:, 6].max() <= 95 and len(set(j[:, 6].tolist())) == 66
    # probabilities that switch a part off
    off = SecondOrder(blur_prob=0, noise_prob=0, final_sinc_prob=0, jpeg_prob=0)
    r = off.draw(50, _gen(1)).numpy()
    assert (r[[0, 1, 3], :, 0] == -1).all() and (r[:, :, 1:3] == 0).all() and (r[2] == 0).all() and not off.has_jpeg and so.has_jpeg
    for kw in ({"blur_prob": 1.5}, {"blur_sigma": (0.0, 1.0)}, {"family_prob": (0.5, 0.5)}, {"family_prob": (0.5, 0.5, 0.5, 0, 0, 0)},
               {"omega": (1.0, 3.5)}, {"omega": (0.0, 1.0)}, {"jpeg_quality": (0, 50)}, {"ksize": 8}, {"bank_size": 0}, {"shot": (-1, 1)},
               {"noise_sigma": (3, 2)}, {"jpeg_chroma": "422"}, {"beta_plateau": (0, 2)}):
        with pytest.raises(ValueError, match="SecondOrder"):
            SecondOrder(**kw)


def test_second_order_bank():
    from srganst.device_data import SecondOrder
    so = SecondOrder(bank_size=300, sinc_bank_size=40, ksize=13)
    bank = so.draw_bank(_gen(2))
    assert bank.dtype == np.float32 and bank.shape == (340, 13, 13) and np.array_equal(bank, so.draw_bank(_gen(2)))
    assert not np.array_equal(bank, so.draw_bank(_gen(3)))
    assert np.abs(bank.astype(np.float64).sum((1, 2)) - 1).max() < 1e-5 and np.isfinite(bank).all()
    neg = (bank < 0).any((1, 2))
    assert neg[300:].all() and 0.03 < neg[:300].mean() < 0.2                        # sinc kernels ring: all of the final section, about 0.1 of the blur section
    # supports: odd, uniform in 7..13 (a narrow kernel's outer weights may underflow to 0 inside its window)
    width = np.array([(np.abs(t).sum(0) > 0).sum() for t in bank])
    assert (width % 2 == 1).all() and width.max() == 13 and {7, 9, 11, 13} <= set(width.tolist())
    assert [so._support(u) for u in (0.0, 0.249, 0.25, 0.5, 0.75, 0.999, 1.0)] == [7, 7, 9, 11, 13, 13, 13]
    assert {SecondOrder(ksize=5)._support(u) for u in (0.0, 0.5, 1.0)} == {5}
    # isotropic kernels are symmetric under transposition, the anisotropic ones are not: 0.45 + 0.12 + 0.12 of the non-sinc
    iso = np.array([np.array_equal(t, t.T) for t in bank[:300][~neg[:300]]])
    assert 0.55 < iso.mean() < 0.85


def test_second_order_fixed():
    from srganst.device_data import SecondOrder
    k = _k()
    table = k.plateau(21, 1.0, 2.0, 0.5, beta=1.5)
    so = SecondOrder.fixed(kernel=table, noise=10.0, shot=0.01, gray=True, key=(5, 6), sinc_omega=2.0, sinc_first=False, jpeg=60)
    bank = so.draw_bank()
    assert bank.shape == (2, 21, 21) and np.array_equal(bank, k.bank([table, k.sinc(21, 2.0)])) and so.has_jpeg
    a, b, j, c = so.draw(3).numpy()
    assert a.tolist() == [[0, int(np.float32(10 / 255).view(np.int32)), int(np.float32(0.01).view(np.int32)), 1, 5, 6, 0, 0]] * 3
    assert b.tolist() == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 3 and c.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]] * 3
    assert j.tolist() == [[0, 0, 0, 0, 0, 0, 60, 0]] * 3
    first = SecondOrder.fixed(sinc_omega=1.5, ksize=7).draw(1).numpy()
    assert first[:, 0, 0].tolist() == [-1, 0, 0, -1] and not SecondOrder.fixed(sinc_omega=1.5).has_jpeg
    none = SecondOrder.fixed()
    assert none.draw_bank().shape == (0, 21, 21) and none.draw(2).numpy()[[0, 1, 3], :, 0].tolist() == [[-1, -1]] * 3
    assert "sinc_omega=2.0" in repr(so) and "jpeg=60" in repr(so) and "final_sinc_prob=0.8" in repr(SecondOrder())
    for kw in (dict(noise=-1.0), dict(shot=float("nan")), dict(jpeg=101), dict(jpeg=50.5), dict(kernel=np.ones((7, 7))),
               dict(sinc_omega=4.0), dict(kernel=np.zeros((21, 21)))):
        with pytest.raises(ValueError):
            SecondOrder.fixed(**kw)


class _ArenaLR(_Arena):
    def __init__(self, sizes, crop, step, out):
        super().__init__(sizes, crop, step)
        self.out = out


def test_loader_draws_per_tile_with_the_second_stage(monkeypatch):
    """A tile's second-stage rows in an epoch depend on neither world size, rank nor batch size; the bank is a function of (seed,
    epoch); the window, transform and first-stage draws are those of the loader without it; with second=None nothing of it runs."""
    from torch.utils.data.distributed import DistributedSampler
    from srganst.device_data import Degradation, DeviceCropLoader, SecondOrder
    arena = _ArenaLR([(60, 70), (40, 90), (33, 35)], 16, 8, out=8)
    deg, so = Degradation(jpeg_prob=0.5), SecondOrder(ksize=7, bank_size=24, sinc_bank_size=8)
    base = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg, second=so)
    plain = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg)
    assert plain.second_draws(1) is None and plain.second is None
    for epoch in (0, 1, 5):
        assert np.array_equal(base.draws(epoch), plain.draws(epoch)) and np.array_equal(base.deg_draws(epoch), plain.deg_draws(epoch))
    (all0, bank0), (all1, bank1) = base.second_draws(0), base.second_draws(1)
    assert all0.shape == (4, len(arena), 8) and bank0.shape == (32, 7, 7)
    assert np.array_equal(all0, base.second_draws(0)[0]) and np.array_equal(bank0, base.second_draws(0)[1])
    assert not np.array_equal(all0, all1) and not np.array_equal(bank0, bank1)
    other = DeviceCropLoader(arena, 2, None, seed=4, degradation=deg, second=so).second_draws(0)
    assert not np.array_equal(all0, other[0]) and not np.array_equal(bank0, other[1])
    by_tile = {}
    for world in (1, 2, 4):
        for batch in (2, 5):
            for rank in range(world):
                sampler = DistributedSampler(arena, world, rank, shuffle=True, seed=11)
                sampler.set_epoch(1)
                ld = DeviceCropLoader(arena, batch, sampler, True, True, seed=3, degradation=deg, second=so)
                ld.set_epoch(1)
                order = np.fromiter(iter(sampler), dtype=np.int64)[: len(ld) * batch]
                desc, rows, rows2, bank = ld.plan_all()
                assert np.array_equal(desc.numpy(), plain.draws(1)[order]) and np.array_equal(rows.numpy(), plain.deg_draws(1)[order])
                assert tuple(rows2.shape) == (4, len(order), 8) and rows2.is_contiguous() and np.array_equal(bank.numpy(), bank1)
                for i, tile in enumerate(order.tolist()):
                    r = rows2[:, i].numpy()
                    assert np.array_equal(by_tile.setdefault(tile, r), r) and np.array_equal(r, all1[:, tile])
    assert len(by_tile) == len(arena)
    with pytest.raises(ValueError, match="needs degradation"):
        DeviceCropLoader(arena, 2, None, second=so)
    with pytest.raises(ValueError, match="half window"):
        DeviceCropLoader(arena, 2, None, degradation=deg, second=SecondOrder(ksize=17))
    # second=None: the rows and generator calls of before - plan_both() with the two private generators, none for a second stage
    made = []
    real = torch.Generator
    monkeypatch.setattr(torch, "Generator", lambda *a, **k: (made.append(1), real(*a, **k))[1])
    desc, rows = plain.plan_both()
    n_plain = len(made)                                  # the RandomSampler's own, the window / transform one, the first stage's
    assert n_plain == 3
    made.clear()
    assert len(base.plan_all()) == 4 and len(made) == n_plain + 2                 # + the second stage's rows and its bank


def test_config_switches():
    from srganst.config import Config
    from srganst.device_data import Degradation, SecondOrder, check_switches
    cfg = Config()
    d = cfg.DATA
    assert d.DEGRADE_SECOND is False and d.VALIDATE_DEGRADE_SINC is None
    assert (d.DEGRADE2_BLUR_PROB, d.DEGRADE2_BLUR_SIGMA, d.DEGRADE2_FAMILY_PROB) == (0.8, (0.2, 1.5), (0.45, 0.25, 0.12, 0.03, 0.12, 0.03))
    assert (d.DEGRADE2_BETA_GAUSSIAN, d.DEGRADE2_BETA_PLATEAU, d.DEGRADE2_SINC_PROB) == ((0.5, 4.0), (1.0, 2.0), 0.1)
    assert (d.DEGRADE2_NOISE_PROB, d.DEGRADE2_NOISE_SIGMA, d.DEGRADE2_SHOT, d.DEGRADE2_SHOT_PROB, d.DEGRADE2_GRAY_PROB) == \
        (1.0, (1.0, 25.0), (1e-5, 0.025), 0.5, 0.4)
    assert (d.DEGRADE2_FINAL_SINC_PROB, d.DEGRADE2_OMEGA, d.DEGRADE2_SINC_FIRST_PROB) == (0.8, (PI / 3, PI), 0.5)
    assert (d.DEGRADE2_JPEG_QUALITY, d.DEGRADE2_JPEG_PROB, d.DEGRADE2_KSIZE, d.DEGRADE2_BANK_SIZE, d.DEGRADE2_SINC_BANK_SIZE) == \
        ((30, 95), 1.0, 21, 1024, 256)
    assert SecondOrder.from_config(cfg) is None
    check_switches(cfg)
    cfg.DATA.DEGRADE_SECOND = True
    with pytest.raises(ValueError, match="DATA.DEGRADE_SECOND needs DATA.DEGRADE"):
        check_switches(cfg)
    cfg.DATA.DEGRADE = cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
    check_switches(cfg)
    assert repr(SecondOrder.from_config(cfg)) == repr(SecondOrder())
    cfg.DATA.DEGRADE2_GRAY_PROB, cfg.DATA.DEGRADE2_KSIZE, cfg.DATA.DEGRADE_JPEG_CHROMA = 0.1, 13, "444"
    got = SecondOrder.from_config(cfg)
    assert (got.gray_prob, got.ksize, got.jpeg_chroma) == (0.1, 13, "444")
    from srganst.validate import _sinc_param
    assert _sinc_param(cfg, None) is None and _sinc_param(cfg, 2) == 2.0
    cfg.DATA.VALIDATE_DEGRADE_SINC = 1.5
    assert _sinc_param(cfg, None) == 1.5 and _sinc_param(cfg, PI) == PI
    for bad in (0.0, -1.0, 3.2):
        with pytest.raises(ValueError, match=r"\(0, pi\]"):
            _sinc_param(cfg, bad)


def test_announce_names_the_second_stage(capsys):
    from srganst.config import Config
    from srganst.device_data import Degradation, SecondOrder, announce_degradation
    cfg = Config()
    announce_degradation(cfg, Degradation())
    assert "DEGRADE_SECOND" not in capsys.readouterr().out
    announce_degradation(cfg, Degradation(), SecondOrder())
    out = capsys.readouterr().out
    assert out.count("DATA.DEGRADE_SECOND: then lr = sinc(jpeg(sinc(quantise(clamp(lr * k2 + n2)))))") == 1 and "gray_prob=0.4" in out


def test_python_refusals():
    from srganst.device_data import filter2d, filter_rows
    x = torch.zeros(1, 3, 16, 16)
    flt = torch.from_numpy(filter_rows([-1], 0, 0, 0, [(0, 0)]))
    with pytest.raises(ValueError, match="ROCm device"):
        filter2d(x, flt, None)
    with pytest.raises(ValueError, match="ROCm device"):
        filter2d(x[0], flt, None)
