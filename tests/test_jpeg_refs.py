"""CPU: the JPEG stage's integer restatement (tests/jpeg_refs.py) - its tables and transform matrix, the int32 range of every
intermediate, its special cases, its independence of the tiling, its closeness to libjpeg from recorded Pillow round trips
(tests/golden/jpeg_pil.npz) - and the host side of the option: Degradation's additional draws, the loader's per-tile draws, the config."""
import os

import numpy as np
import pytest
import torch

import jpeg_refs as refs
from conftest import ROOT
from test_degrade_refs import _Arena

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")
SIZES = ((24, 24), (17, 13), (8, 8), (48, 40), (9, 31), (3, 20))
QUALITIES = (10, 30, 50, 75, 90, 95)


def _image(h, w, seed=0):
    """A smooth image with an edge and some noise, on the 1/255 grid: fp32 [3, h, w]."""
    return refs.fixture_image(h, w, seed).transpose(2, 0, 1).astype(np.float32) / np.float32(255)


def test_table_rule():
    for Q, s in ((1, 5000), (10, 500), (49, 102), (50, 100), (75, 50), (100, 0)):
        lum, chrom = refs.tables(Q)
        for got, base in ((lum, refs.LUMA), (chrom, refs.CHROMA)):
            assert got.shape == (8, 8) and np.array_equal(got, np.clip((base * s + 50) // 100, 1, 255))
    assert all((t == 1).all() for t in refs.tables(100))
    assert all((t == 255).all() for t in refs.tables(1))                     # 16 * 50 = 800 -> clamped
    assert np.array_equal(refs.tables(50)[0], refs.LUMA) and np.array_equal(refs.tables(50)[1], refs.CHROMA)
    assert refs.tables(75)[0][0].tolist() == [8, 6, 5, 8, 12, 20, 26, 31]    # libjpeg's quality-75 luminance row 0
    z = np.load(GOLDEN)                                                      # libjpeg's own tables, from the recorded files
    for Q in QUALITIES:
        assert np.array_equal(np.stack(refs.tables(Q)).reshape(2, 64), z[f"qt_q{Q}"]), Q


def test_transform_matrix_against_fp64():
    C, T = refs.dct_matrix_f64(), refs.transform_matrix()
    assert np.abs(C @ C.T - np.eye(8)).max() < 1e-15
    assert T.dtype == np.int64 and np.abs(T - 8192 * C).max() <= 0.5 and (T[0] == 2896).all() and np.abs(T).max() == 4017
    # T = 8192 C + e, |e| <= 0.5, rows of C have sum |C| <= sqrt(8): |T T^t / 8192^2 - I| <= (2 * 0.5 * sqrt(8) * 8192 + 8 * 0.25) / 8192^2
    assert np.abs(T @ T.T / 8192.0 ** 2 - np.eye(8)).max() <= (np.sqrt(8) * 8192 + 2) / 8192.0 ** 2
    # the kernel's 24-bit multiplies: every operand bound of DESIGN section 22 is below 2^23
    assert np.abs(T).sum(1).max() == 8 * 2896 and 8 * 2896 * 36000 < 2 ** 31


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_every_intermediate_fits_int32(chroma):
    """0/255 checkerboards of three periods and random 0/255 images at Q = 1, 50, 100: _i32 asserts inside the restatement."""
    refs.PEAK[0] = 0
    g = np.random.default_rng(5)
    images = [refs.checkerboard(32, 32, p) for p in (1, 2, 4)] + [g.integers(0, 2, (3, 24, 40)).astype(np.float32) for _ in range(3)]
    for x in images:
        for Q in (1, 50, 100):
            out = refs.jpeg_sample(x, Q, chroma)
            assert out.shape == x.shape and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
            assert np.array_equal(np.rint(out * 255).astype(np.float32) / np.float32(255), out)        # on the grid
    print(f"[jpeg {chroma}] peak intermediate {refs.PEAK[0]:.3e}")
    assert 1e6 < refs.PEAK[0] < 2 ** 31


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_special_cases(chroma):
    x = _image(17, 13)
    off = x + np.float32(0.3 / 255)                                          # off the grid
    assert refs.same(refs.jpeg_sample(off, 0, chroma), off)                  # Q = 0: the bits
    for Q in (-1, 101, 1 << 20):
        assert np.isnan(refs.jpeg_sample(x, Q, chroma)).all()
    # off the grid and outside [0, 1]: the codec sees rint(255 clamp01(v))
    wild = (x - 0.5) * 3
    assert refs.same(refs.jpeg_sample(wild, 60, chroma), refs.jpeg_sample(np.rint(255 * np.clip(wild, 0, 1)) / 255, 60, chroma))
    # a non-finite element: its MCU is NaN in all three channels, nothing else moves
    M = 8 if chroma == "444" else 16
    x = _image(33, 40)
    clean = refs.jpeg_sample(x, 50, chroma)
    for bad, (c, y, xx) in ((np.nan, (1, 9, 20)), (np.inf, (0, 32, 39)), (-np.inf, (2, 0, 0))):
        dirty = x.copy()
        dirty[c, y, xx] = bad
        out = refs.jpeg_sample(dirty, 50, chroma)
        mask = np.zeros(x.shape, bool)
        mask[:, y // M * M:y // M * M + M, xx // M * M:xx // M * M + M] = True
        assert np.isnan(out[mask]).all() and np.array_equal(out[~mask], clean[~mask])


def test_quality_100_is_nearly_lossless():
    """Q = 100, 444: all-ones tables; what is left is the colour transform's and the DCT's rounding - at most 3 levels on the test
    image (the fixtures' image at their six sizes, its noise seeded by H * W + q with q = 100 as for every other quality)."""
    for h, w in SIZES:
        x = _image(h, w, 100)
        d = np.abs(np.rint(255 * refs.jpeg_sample(x, 100, "444")) - np.rint(255 * x)).max()
        print(f"[jpeg Q 100 444 {h}x{w}] max pixel change {d:g} levels")
        assert d <= 3


@pytest.mark.parametrize("chroma", ["444", "420"])
@pytest.mark.parametrize("h, w", [(33, 40), (70, 50), (17, 13), (1, 1)])
def test_result_does_not_depend_on_the_tiling(chroma, h, w):
    x = _image(h, w, 3)
    whole = refs.jpeg_sample(x, 40, chroma)
    for tile in (16, refs.TILE, 48):
        assert refs.same(refs.jpeg_sample(x, 40, chroma, tile=tile), whole), tile
    # and a batch is its samples
    deg = np.zeros((3, 8), np.int32)
    deg[:, 6] = (40, 0, 101)
    out = refs.jpeg_reference(np.stack([x, x, x]), deg, chroma, tile=refs.TILE)
    assert refs.same(out[0], whole) and refs.same(out[1], x) and np.isnan(out[2]).all()


def test_closeness_to_libjpeg():
    """Against Pillow's round trips: in every case rms(ours - Pillow) < rms(Pillow - input).  A sanity bound on the MODEL (nearest
    chroma upsampling, no fancy filter; an integer DCT): not to be tightened to the measured ratios, which DESIGN section 22 records."""
    z = np.load(GOLDEN)
    worst = {"444": 0.0, "420": 0.0}
    for H, W in SIZES:
        for q in QUALITIES:
            img = z[f"in_{H}x{W}_q{q}"]
            assert np.array_equal(img, refs.fixture_image(H, W, q))
            x = img.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            for mode, sub in (("444", 0), ("420", 2)):
                pil = z[f"out_{H}x{W}_q{q}_s{sub}"].astype(np.float64)
                ours = np.rint(255 * refs.jpeg_sample(x, q, mode).astype(np.float64)).transpose(1, 2, 0)
                ours_err, pil_err = np.sqrt(((ours - pil) ** 2).mean()), np.sqrt(((pil - img) ** 2).mean())
                assert ours_err < pil_err, (H, W, q, mode, ours_err, pil_err)
                worst[mode] = max(worst[mode], ours_err / pil_err)
    print(f"[jpeg vs libjpeg] worst rms(ours - Pillow) / rms(Pillow - input): 444 {worst['444']:.3f}, 420 {worst['420']:.3f}")
    assert len(z.files) == len(SIZES) * len(QUALITIES) * 3 + len(QUALITIES)


def test_draws_with_and_without_jpeg():
    from srganst.device_data import Degradation, degrade_rows
    gen = lambda s: torch.Generator().manual_seed(s)
    n = 3000
    base = Degradation((0.5, 3.0), True, 0.7, (2.0, 20.0), 0.6, 15)
    # jpeg_prob = 0: the draw of before, bit for bit (rand [n, 6] then randint [n, 2], nothing else), and zero words
    g = gen(4)
    u = torch.rand(n, 6, generator=g, dtype=torch.float64)
    keys = torch.randint(0, 1 << 32, (n, 2), generator=g, dtype=torch.int64)
    g2 = gen(4)
    rows0 = base.draw(n, g2)
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=g2))          # the generator is where it was left before
    assert bool((rows0[:, 6:] == 0).all()) and np.array_equal(rows0[:, 4:6].numpy().view(np.uint32), keys.numpy().astype(np.uint32))
    s1 = 0.5 + 2.5 * u[:, 0].numpy()
    assert np.array_equal(rows0.numpy(), degrade_rows(np.where(u[:, 3] < 0.7, s1, 0), np.where(u[:, 3] < 0.7, 0.5 + 2.5 * u[:, 1].numpy(), 0),
                                                      np.pi * u[:, 2].numpy(), np.where(u[:, 5] < 0.6, 2 + 18 * u[:, 4].numpy(), 0), keys.numpy()))
    assert torch.equal(rows0, Degradation((0.5, 3.0), True, 0.7, (2.0, 20.0), 0.6, 15, (10, 20), 0.0, "444").draw(n, gen(4)))
    # jpeg_prob = 1: the first six words unchanged, word 6 a quality in the closed range (both ends drawn), word 7 zero
    on = Degradation((0.5, 3.0), True, 0.7, (2.0, 20.0), 0.6, 15, jpeg_quality=(30, 33), jpeg_prob=1.0).draw(n, gen(4))
    assert torch.equal(on[:, :6], rows0[:, :6]) and bool((on[:, 7] == 0).all())
    assert sorted(set(on[:, 6].tolist())) == [30, 31, 32, 33]
    half = Degradation(jpeg_prob=0.5).draw(n, gen(7))
    assert torch.equal(half[:, :6], Degradation().draw(n, gen(7))[:, :6])
    q = half[:, 6].numpy()
    assert abs((q == 0).mean() - 0.5) < 0.05 and q[q > 0].min() >= 30 and q[q > 0].max() <= 95 and len(set(q.tolist())) > 50
    # fixed rows and the repr
    assert Degradation.fixed(0, 0, 0, 0, (3, 4), jpeg=40).draw(2).tolist() == [[-1082130432, 0, 0, 0, 3, 4, 40, 0]] * 2
    assert degrade_rows([1], [1], [0], [0], [(1, 2)], jpeg=[77])[0, 6:].tolist() == [77, 0]
    assert "jpeg" not in repr(Degradation()) and "jpeg" not in repr(Degradation.fixed(1, 1, 0, 0))
    assert repr(Degradation(jpeg_prob=0.25, jpeg_chroma="444")).endswith("ksize=21, jpeg_quality=(30, 95), jpeg_prob=0.25, jpeg_chroma='444')")
    assert repr(Degradation.fixed(1, 1, 0, 0, jpeg=40)).endswith("ksize=21, jpeg=40, jpeg_chroma='420')")
    assert not Degradation().has_jpeg and Degradation(jpeg_prob=0.1).has_jpeg
    assert Degradation.fixed(1, 1, 0, 0, jpeg=5).has_jpeg and not Degradation.fixed(1, 1, 0, 0).has_jpeg
    for kw in ({"jpeg_quality": (0, 50)}, {"jpeg_quality": (60, 50)}, {"jpeg_quality": (50, 101)}, {"jpeg_quality": (30.5, 95)},
               {"jpeg_prob": 1.5}, {"jpeg_prob": -0.1}, {"jpeg_chroma": "422"}):
        with pytest.raises(ValueError):
            Degradation(**kw)
    for bad in (-1, 101, 50.5):
        with pytest.raises(ValueError, match="0..100"):
            Degradation.fixed(1, 1, 0, 0, jpeg=bad)


def test_loader_draws_per_tile_with_jpeg():
    """A tile's quality in an epoch depends on neither world size, rank nor batch size; its other words are those of the loader
    without the JPEG stage."""
    from torch.utils.data.distributed import DistributedSampler
    from srganst.device_data import Degradation, DeviceCropLoader
    arena = _Arena([(60, 70), (40, 90), (33, 35)], 16, 8)
    with_jpeg, without = Degradation(jpeg_prob=0.7, jpeg_quality=(5, 100)), Degradation()
    base = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=with_jpeg)
    plain = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=without)
    all1 = base.deg_draws(1)
    assert np.array_equal(all1[:, :6], plain.deg_draws(1)[:, :6]) and (plain.deg_draws(1)[:, 6:] == 0).all()
    assert (all1[:, 6] > 0).any() and (all1[:, 6] == 0).any() and not np.array_equal(all1[:, 6], base.deg_draws(0)[:, 6])
    by_tile = {}
    for world in (1, 2):
        for batch in (2, 5):
            for rank in range(world):
                sampler = DistributedSampler(arena, world, rank, shuffle=True, seed=11)
                sampler.set_epoch(1)
                ld = DeviceCropLoader(arena, batch, sampler, True, True, seed=3, degradation=with_jpeg)
                ld.set_epoch(1)
                order = np.fromiter(iter(sampler), dtype=np.int64)[: len(ld) * batch]
                desc, rows = ld.plan_both()
                assert np.array_equal(desc.numpy(), plain.draws(1)[order])
                for tile, row in zip(order.tolist(), rows.numpy()):
                    assert np.array_equal(by_tile.setdefault(tile, row), row) and np.array_equal(row, all1[tile])
    assert len(by_tile) == len(arena)


def test_config_defaults_and_switches():
    from srganst.config import Config
    from srganst.device_data import Degradation, check_switches
    cfg = Config()
    d = cfg.DATA
    assert (d.DEGRADE_JPEG_PROB, d.DEGRADE_JPEG_QUALITY, d.DEGRADE_JPEG_CHROMA, d.VALIDATE_DEGRADE_JPEG) == (0.0, (30, 95), "420", None)
    cfg.DATA.DEGRADE = cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
    assert repr(Degradation.from_config(cfg)) == repr(Degradation()) and not Degradation.from_config(cfg).has_jpeg
    cfg.DATA.DEGRADE_JPEG_PROB, cfg.DATA.DEGRADE_JPEG_QUALITY, cfg.DATA.DEGRADE_JPEG_CHROMA = 0.5, (40, 90), "444"
    check_switches(cfg)
    got = Degradation.from_config(cfg)
    assert got.has_jpeg and (got.jpeg_prob, got.jpeg_quality, got.jpeg_chroma) == (0.5, (40, 90), "444")
    cfg.DATA.DEGRADE = False
    with pytest.raises(ValueError, match="DATA.DEGRADE_JPEG_PROB needs DATA.DEGRADE"):
        check_switches(cfg)
    from srganst.validate import _jpeg_param
    assert _jpeg_param(cfg, None) is None and _jpeg_param(cfg, 40) == 40
    cfg.DATA.VALIDATE_DEGRADE_JPEG = 75
    assert _jpeg_param(cfg, None) == 75 and _jpeg_param(cfg, 10) == 10
    for bad in (0, 101, 40.5):
        with pytest.raises(ValueError, match="1..100"):
            _jpeg_param(cfg, bad)
