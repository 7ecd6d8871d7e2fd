"""CPU: the degradation stage's fp64 restatement (tests/degrade_refs.py) against known answers and an independent torch formulation,
the Gaussian's parametrisation, Degradation.draw, the loader's per-tile draws and the config switches."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_refs as refs

# the GPU cases of tests/test_degrade_gpu.py: (S, scale, K) and the kernels (sigma1, sigma2, theta_deg)
CROP_CASES = [(12, 4, 21), (24, 4, 3), (24, 4, 5), (24, 4, 21), (32, 8, 9), (8, 2, 7)]
KERNELS = [(0.2, 0.2, 0.0), (4.0, 4.0, 0.0), (0.6, 3.5, 30.0)]


def _fixed(s1, s2, th, noise, key, n=1, ksize=21):
    from srganst.device_data import Degradation
    return Degradation.fixed(s1, s2, th, noise, key, ksize=ksize).draw(n).numpy()


def test_philox_known_answer():
    """Random123's kat_vectors, philox4x32 10 rounds: zero counter and key, and the all-ones and pi-digits vectors."""
    out = refs.philox4x32([0, 0, 0, 0], (0, 0))
    assert [int(v) for v in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = refs.philox4x32([0xffffffff] * 4, (0xffffffff, 0xffffffff))
    assert [int(v) for v in out] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    out = refs.philox4x32([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0))
    assert [int(v) for v in out] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    z = refs.gauss(200000, 123, 456)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01 and np.isfinite(z).all()


@pytest.mark.parametrize("H, W, scale, K", [(24, 24, 4, 21), (23, 30, 4, 21), (9, 11, 2, 7), (32, 32, 8, 9), (12, 12, 4, 21)])
def test_restatement_against_torch(H, W, scale, K):
    """F.pad(reflect) -> F.conv2d in fp64 -> Bicubic("cpu") without its rounding, built from its own tables in fp64."""
    from srganst.bicubic import Bicubic
    g = torch.Generator().manual_seed(H * W)
    gt = (torch.randint(0, 256, (3, 3, H, W), generator=g).float() / 255)
    deg = np.concatenate([_fixed(0.6, 3.5, 30.0, 0.0, 1, ksize=K), _fixed(4.0, 4.0, 0.0, 0.0, 2, ksize=K), _fixed(0, 0, 0, 0.0, 3, ksize=K)])
    ref = refs.degrade_reference(gt.numpy(), deg, scale, K, quantise=False)
    p = K // 2
    bic = Bicubic("cpu")
    w0, i0, w1, i1 = bic.tables(H, W, 1.0 / scale, "cpu")
    for b in range(3):
        qa, qb, qc, _, _, _ = refs.unpack(deg[b])
        x = gt[b:b + 1].double()
        if not qa < 0:
            k = torch.from_numpy(refs.weights(qa, qb, qc, K))
            assert abs(float(k.sum()) - 1) < 1e-14 and float(k.min()) >= 0
            xp = F.pad(x, (p, p, p, p), mode="reflect")
            x = F.conv2d(xp.reshape(3, 1, H + 2 * p, W + 2 * p), k.reshape(1, 1, K, K)).reshape(1, 3, H, W)
        v = (x[:, :, i0, :] * w0.double()[None, None, :, :, None]).sum(3)                     # Bicubic.forward's two passes
        v = (v.permute(0, 1, 3, 2)[:, :, i1, :] * w1.double()[None, None, :, :, None]).sum(3).permute(0, 1, 3, 2)
        assert float((v[0] - torch.from_numpy(ref[b])).abs().max()) < 1e-13
    # the identity sample, rounded, is the CPU Bicubic's own result up to its fp32 arithmetic
    idn = refs.degrade_reference(gt.numpy(), deg, scale, K)[2]
    assert float((torch.from_numpy(idn) - bic(gt[2:3], scale=1.0 / scale)[0].double()).abs().max()) <= 1 / 255 + 1e-7


def test_kernel_parametrisation():
    """q = (A/2, B, C/2) of the inverse covariance, x = columns, y = rows: equal sigmas give one kernel at every theta; a quarter
    turn of theta is the kernel's quarter turn - its transpose, flipped - and for an axis-aligned kernel its transpose."""
    K = 21

    def kern(s1, s2, th):
        qa, qb, qc, *_ = refs.unpack(_fixed(s1, s2, th, 0, 0)[0])
        return refs.weights(qa, qb, qc, K)
    k0 = kern(2.0, 2.0, 0.0)
    for th in (17.0, 45.0, 90.0, 133.0):
        assert np.abs(kern(2.0, 2.0, th) - k0).max() < 1e-8
    assert np.abs(kern(0.6, 3.5, 90.0) - kern(0.6, 3.5, 0.0).T).max() < 1e-8
    assert np.abs(kern(0.6, 3.5, 120.0) - np.rot90(kern(0.6, 3.5, 30.0))).max() < 1e-8
    assert np.abs(kern(0.6, 3.5, 120.0) - kern(0.6, 3.5, 30.0).T[::-1]).max() < 1e-8
    assert np.abs(kern(0.6, 3.5, 120.0) - kern(3.5, 0.6, 30.0)).max() < 1e-8
    # theta = 0: sigma1 along x (columns)
    k = kern(0.6, 3.5, 0.0)
    assert k[10, 11] < k[11, 10]
    # second moments of a kernel well inside its window: the covariance R diag(s1^2, s2^2) R^T
    k = kern(1.0, 2.0, 30.0)
    d = np.arange(-10, 11.0)
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    cov = np.array([[c * c * 1 + s * s * 4, c * s * (1 - 4)], [c * s * (1 - 4), s * s * 1 + c * c * 4]])
    mxx, myy, mxy = (k * d[None, :] ** 2).sum(), (k * d[:, None] ** 2).sum(), (k * d[None, :] * d[:, None]).sum()
    assert np.allclose([mxx, mxy, myy], [cov[0, 0], cov[0, 1], cov[1, 1]], atol=2e-3)
    # the sentinel
    assert refs.unpack(_fixed(0, 0, 0, 5.0, 7)[0])[0] < 0 and refs.unpack(_fixed(0, 0, 0, 5.0, 7)[0])[3] == np.float32(5 / 255)
    assert _fixed(0, 0, 0, 0, (3, 4))[0].tolist()[4:] == [3, 4, 0, 0]


def test_draw_ranges_probabilities_and_reproducibility():
    from srganst.device_data import Degradation
    n = 4000
    gen = lambda s: torch.Generator().manual_seed(s)
    d = Degradation((0.5, 3.0), True, 1.0, (2.0, 20.0), 1.0, 15)
    rows = d.draw(n, gen(1))
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (n, 8) and bool((rows[:, 6:] == 0).all())
    q = rows[:, :4].numpy().copy().view(np.float32).astype(np.float64)
    # eigenvalues of [[2qa, qb], [qb, 2qc]] are 1/sigma^2
    tr, det = 2 * q[:, 0] + 2 * q[:, 2], 4 * q[:, 0] * q[:, 2] - q[:, 1] ** 2
    disc = np.sqrt(np.maximum(tr * tr / 4 - det, 0))
    s_small, s_big = 1 / np.sqrt(tr / 2 + disc), 1 / np.sqrt(tr / 2 - disc)
    assert s_small.min() >= 0.5 - 1e-5 and s_big.max() <= 3.0 + 1e-4 and s_small.min() < 0.6 and s_big.max() > 2.8
    assert (s_big - s_small).max() > 1.0                                  # anisotropic
    sn = q[:, 3] * 255
    assert sn.min() >= 2.0 - 1e-4 and sn.max() <= 20.0 + 1e-4 and sn.min() < 2.5 and sn.max() > 19.5
    assert len(np.unique(rows[:, 4:6].numpy(), axis=0)) == n
    iso = Degradation((0.5, 3.0), False).draw(n, gen(1))[:, :4].numpy().copy().view(np.float32)
    assert np.abs(iso[:, 1]).max() < 1e-6 and np.allclose(iso[:, 0], iso[:, 2], rtol=1e-6)
    none = Degradation(blur_prob=0.0, noise_prob=0.0).draw(n, gen(2))
    assert not refs.is_degraded(none.numpy()).any()
    qn = Degradation(blur_prob=0.0).draw(n, gen(2))[:, :4].numpy().copy().view(np.float32)
    assert (qn[:, 0] < 0).all() and (qn[:, 3] > 0).any()
    half = Degradation(blur_prob=0.5, noise_prob=0.25).draw(n, gen(3))[:, :4].numpy().copy().view(np.float32)
    assert abs((half[:, 0] < 0).mean() - 0.5) < 0.05 and abs((half[:, 3] == 0).mean() - 0.75) < 0.05
    assert torch.equal(d.draw(n, gen(5)), d.draw(n, gen(5))) and not torch.equal(d.draw(n, gen(5)), d.draw(n, gen(6)))
    for kw in ({"ksize": 4}, {"ksize": 23}, {"ksize": 1}, {"blur_sigma": (0.0, 1.0)}, {"blur_sigma": (2.0, 1.0)}, {"noise_sigma": (-1, 2)},
               {"blur_prob": 1.5}, {"noise_prob": -0.1}):
        with pytest.raises(ValueError):
            Degradation(**kw)
    with pytest.raises(ValueError):
        Degradation.fixed(1.0, 0.0, 0, 0)


class _Arena:
    """What DeviceCropLoader reads of an arena, on the host."""
    def __init__(self, sizes, crop, step):
        from srganst.device_data import tile_grid
        self.table_host = np.array([(0, h, w) for h, w in sizes], np.int64)
        self.crop, self.device = crop, torch.device("cpu")
        self.tiles = tile_grid(sizes, crop, step)
        self.n_images = len(sizes)

    def __len__(self):
        return len(self.tiles)

    def check_desc(self, desc):
        pass


def test_loader_draws_per_tile():
    """A tile's deg row in an epoch depends on neither world size, rank nor batch size; epochs differ and repeat; the window and
    transform draws are those of the loader without a degradation."""
    from torch.utils.data.distributed import DistributedSampler
    from srganst.device_data import Degradation, DeviceCropLoader
    arena = _Arena([(60, 70), (40, 90), (33, 35)], 16, 8)
    deg = Degradation()
    base = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg)
    plain = DeviceCropLoader(arena, 2, None, True, True, seed=3)
    for epoch in (0, 1, 5):
        assert np.array_equal(base.draws(epoch), plain.draws(epoch))
        assert plain.deg_draws(epoch) is None
    all0, all1 = base.deg_draws(0), base.deg_draws(1)
    assert all0.shape == (len(arena), 8) and np.array_equal(all0, base.deg_draws(0)) and not np.array_equal(all0, all1)
    assert not np.array_equal(all0, DeviceCropLoader(arena, 2, None, seed=4, degradation=deg).deg_draws(0))
    by_tile = {}
    for world in (1, 2, 4):
        for batch in (2, 5):
            for rank in range(world):
                sampler = DistributedSampler(arena, world, rank, shuffle=True, seed=11)
                sampler.set_epoch(1)
                ld = DeviceCropLoader(arena, batch, sampler, True, True, seed=3, degradation=deg)
                ld.set_epoch(1)
                order = np.fromiter(iter(sampler), dtype=np.int64)[: len(ld) * batch]
                desc, rows = ld.plan_both()
                assert rows.shape == (len(order), 8) and np.array_equal(desc.numpy(), plain.draws(1)[order])
                for tile, row in zip(order.tolist(), rows.numpy()):
                    assert np.array_equal(by_tile.setdefault(tile, row), row) and np.array_equal(row, all1[tile])
    assert len(by_tile) == len(arena)
    with pytest.raises(ValueError, match="half window"):
        DeviceCropLoader(_Arena([(20, 20)], 8, 8), 1, None, degradation=deg)


def test_check_switches_and_config_defaults():
    from srganst.config import Config
    from srganst.device_data import Degradation, check_switches
    cfg = Config()
    d = cfg.DATA
    assert (d.DEGRADE, d.DEGRADE_BLUR_SIGMA, d.DEGRADE_BLUR_ANISO, d.DEGRADE_BLUR_PROB, d.DEGRADE_BLUR_KSIZE, d.DEGRADE_NOISE_SIGMA,
            d.DEGRADE_NOISE_PROB, d.VALIDATE_DEGRADE) == (False, (0.2, 4.0), True, 1.0, 21, (0.0, 25.0), 1.0, None)
    check_switches(cfg)
    assert Degradation.from_config(cfg) is None
    cfg.DATA.DEGRADE = True
    for on_device in (False, True):
        cfg.DATA.ON_DEVICE = on_device
        with pytest.raises(ValueError, match="DATA.DEGRADE needs DATA.ON_DEVICE_WHOLE_IMAGES"):
            check_switches(cfg)
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
    check_switches(cfg)
    assert repr(Degradation.from_config(cfg)) == repr(Degradation())


def test_quantised_rule_on_a_perturbed_reference():
    """The quantised rule of the GPU tests, exercised without a GPU: a stand-in for the kernel that is off by the whole bound, the
    reference moved by +3e-5 or by -3e-5 before clamping and rounding, passes the rule in every case, and over the GPU tests' inputs
    under 1 % of its pixels differ from the reference's own rounding (255 * 3e-5 = 0.77 % of a grid step) - the reference alone
    decides which.  A stand-in that is a whole grid step off is refused."""
    from srganst.device_data import crops_reference
    for sign in (1.0, -1.0):
        n = differ = 0
        for S, scale, K in CROP_CASES:
            imgs = refs.arena_images(S)
            desc = refs.arena_descriptors(imgs, S)
            gt, _ = crops_reference(imgs, desc, S, scale)
            for s1, s2, th in KERNELS:
                for noise in (0.0, 25.0):
                    deg = _fixed(s1, s2, th, noise, 5, n=len(desc), ksize=K)
                    ref = refs.degrade_reference(gt.numpy(), deg, scale, K, quantise=False)
                    stand_in = np.rint(255.0 * np.clip(ref + sign * refs.BOUND, 0, 1)).astype(np.float32) / np.float32(255)
                    differ += refs.check_quantised(stand_in, ref, deg, f"S {S} x{scale} K {K} perturbed by {sign * refs.BOUND:+.0e}")
                    n += ref.size
                    off = np.rint(255.0 * np.clip(ref, 0, 1)) + 1
                    with pytest.raises(AssertionError):
                        refs.check_quantised((off / 255).astype(np.float32), ref, deg, "one step off")
        assert 0 < differ < 0.01 * n, (sign, differ, n)
