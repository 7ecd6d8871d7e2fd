"""CPU: the host side of the resize round trip - the fp64 restatement of sst_rescale in tests/resize_refs.py
against torch, the rows and draws of srganst.device_data (rescale_rows, SecondOrder(resize_prob=...), DeviceCropLoader) and the config
switches."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filter_refs
import resize_refs as refs
from test_filter_refs import _ArenaLR

TORCH_MODE = {0: "area", 1: "bilinear", 2: "bicubic"}


# ---- the restatement
@pytest.mark.parametrize("h, w", [(24, 24), (7, 9), (33, 40), (2, 2)])
def test_axis_matrices_against_torch_in_fp64(h, w):
    """Every intermediate height from ceil(h / 4) to 2 h (the width scaled alike, within its own limits), the three modes, to a size
    and back: within 1e-12 of F.interpolate(size=...) in fp64."""
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.rand(1, 3, h, w, generator=g, dtype=torch.float64)
    worst = 0.0
    for hi in range(-(-h // 4), 2 * h + 1):
        wi = min(max(int(w * hi / h), -(-w // 4)), 2 * w)
        for mode in (0, 1, 2):
            kw = {} if mode == 0 else {"align_corners": False}
            want = F.interpolate(x, size=(hi, wi), mode=TORCH_MODE[mode], **kw)
            got = refs.resize(x[0].numpy(), (hi, wi), mode)
            worst = max(worst, float(np.abs(got - want[0].numpy()).max()))
            back = F.interpolate(want, size=(h, w), mode=TORCH_MODE[mode], **kw)
            worst = max(worst, float(np.abs(refs.resize(want[0].numpy(), (h, w), mode) - back[0].numpy()).max()))
    print(f"axis matrices {h}x{w}: max |restatement - F.interpolate| = {worst:.3g}")
    assert worst <= 1e-12


def test_equal_size_is_the_identity_bit_for_bit():
    for n in (1, 2, 7, 24, 33):
        for mode in (0, 1, 2):
            M = refs.axis_matrix(mode, n, n).astype(np.float32)
            assert np.array_equal(M, np.eye(n, dtype=np.float32)), (n, mode)
    x = np.random.default_rng(0).random((3, 7, 9)).astype(np.float32)
    for mode in (0, 1, 2):
        assert np.array_equal(refs.resize(x.astype(np.float64), (7, 9), mode).astype(np.float32), x)


def test_matrix_rows_tap_counts_and_weight_sums():
    """What the bound assumes: rows sum to 1, at most TAPS taps, sum|w| <= S_ABS, within the size limits of the kernel."""
    for n_in in (2, 7, 24, 33, 65):
        for n_out in range(-(-n_in // 4), 2 * n_in + 1):
            for a, b in ((n_in, n_out), (n_out, n_in)):                   # to the intermediate size, and back
                for mode in (0, 1, 2):
                    M = refs.axis_matrix(mode, a, b)
                    assert np.abs(M.sum(1) - 1).max() < 1e-14
                    assert np.abs(M).sum(1).max() <= refs.S_ABS[mode] + 1e-14 and (M != 0).sum(1).max() <= refs.TAPS[mode]


def test_noise_rule_is_the_filter_stage_s():
    from srganst.device_data import filter_rows, rescale_rows
    x = np.random.default_rng(1).random((1, 3, 6, 5)).astype(np.float32)
    for noise, shot, gray in ((10.0, 0.0, 0), (0.0, 0.02, 1), (4.0, 0.01, 0)):
        flt = filter_rows([-1], noise, shot, gray, [(7, 8)])
        rows = rescale_rows(None, ("area", "area"), noise, shot, gray, [(7, 8)])
        want = filter_refs.filter_reference(x, flt, None, quantise=False)
        assert np.array_equal(refs.rescale_reference(x, rows, quantise=False), want)
        rows = rescale_rows([(6, 5)], ("bicubic", "bilinear"), noise, shot, gray, [(7, 8)])          # the identity resize
        assert np.abs(refs.rescale_reference(x, rows, quantise=False) - want).max() < 1e-15
    v = np.full((3, 4, 4), 0.5)
    z = filter_refs.gauss_at(np.arange(48, dtype=np.uint64).reshape(3, 4, 4), 3, 9)
    assert np.array_equal(refs.noise_at(v, 0.1, 0.0, 0, 3, 9), v + 0.1 * z)
    assert np.array_equal(refs.noise_at(v, 0.1, 0.0, 1, 3, 9), v + 0.1 * z[:1])


def test_bound_grows_with_what_it_models():
    from srganst.device_data import rescale_rows
    b = lambda size, modes, noise=0.0, shot=0.0: float(refs.bound(rescale_rows([size], modes, noise, shot, 0, [(1, 2)]))[0])
    assert b(None, ("area", "area")) == 0.0
    assert 0 < b((12, 12), ("bilinear", "bilinear")) < b((12, 12), ("area", "area")) < b((12, 12), ("bicubic", "bicubic")) < 2e-4
    assert b((12, 12), ("bicubic", "bicubic")) < b((12, 12), ("bicubic", "bicubic"), 10.0) < b((12, 12), ("bicubic", "bicubic"), 10.0, 0.02)
    assert b(None, ("area", "area"), 10.0) == pytest.approx(16 * refs.U * 5.9 * 10 / 255 + refs.U * (1 + 5.9 * 10 / 255), rel=1e-6)


# ---- the rows
def test_rescale_rows_words_and_refusals():
    from srganst.device_data import rescale_rows
    rows = rescale_rows([None, 0, (5, 9), (48, 12)], [("area", "area"), ("bicubic", "area"), ("bilinear", "bicubic"), ("bicubic", "bicubic")],
                        [0.0, 25.5, 0.0, 2.55], [0.0, 0.0, 0.02, 0.01], [0, 1, 1, 0], [(1, 2), (3, 4), (0xFFFFFFFF, 5), (6, 0x80000000)])
    assert rows.dtype == np.int32 and rows.shape == (4, 8) and not rows[:, 7].any()
    assert rows[:, :2].tolist() == [[0, 0], [0, 0], [5, 9], [48, 12]]
    assert np.array_equal(rows[:, 2].view(np.float32), np.float32([0, 0.1, 0, 0.01]))
    assert np.array_equal(rows[:, 3].view(np.float32), np.float32([0, 0, 0.02, 0.01]))
    assert rows[:, 4:6].view(np.uint32).tolist() == [[1, 2], [3, 4], [0xFFFFFFFF, 5], [6, 0x80000000]]
    assert rows[:, 6].tolist() == [0, 2 | 0 << 2 | 16, 1 | 2 << 2 | 16, 2 | 2 << 2]
    assert [refs.unpack(r)[6:9] for r in rows] == [(0, 0, 0), (2, 0, 1), (1, 2, 1), (2, 2, 0)]
    one = rescale_rows(None, ("bilinear", "area"), 1.0, 0.0, 0, [(1, 2), (3, 4)])                      # broadcast forms
    assert one.shape == (2, 8) and not one[:, :2].any() and one[:, 6].tolist() == [1, 1]
    assert not rescale_rows(0, ("area", "area"), 0, 0, 0, [(1, 2)])[:, :4].any()
    ok = dict(size=[(4, 4)], modes=("area", "area"), noise255=1.0, shot=0.0, gray=0, keys=[(1, 2)])
    for bad, match in ((dict(noise255=-1.0), "finite and >= 0"), (dict(noise255=float("nan")), "finite and >= 0"),
                       (dict(shot=-0.1), "finite and >= 0"), (dict(shot=float("inf")), "finite and >= 0"), (dict(gray=2), "gray must be 0 or 1"),
                       (dict(modes=("nearest", "area")), "modes must be pairs"), (dict(modes=[("area",)]), "modes must be pairs"),
                       (dict(modes=[("area", "area")] * 2), "2 mode pairs for 1 keys"), (dict(size=[(4, 4), (4, 4)]), "2 sizes for 1 keys"),
                       (dict(size=[(4, 0)]), "two positive integers"), (dict(size=[(-4, 4)]), "two positive integers"),
                       (dict(size=[(4.5, 4)]), "pair of integers"), (dict(size=[(4, 4, 4)]), "pair of integers")):
        with pytest.raises(ValueError, match=match):
            rescale_rows(**{**ok, **bad})


# ---- the draws
def test_draw_resize_sizes_kinds_and_modes():
    from srganst.device_data import RESIZE_MODES, SecondOrder
    so = SecondOrder(resize_prob=(0.3, 0.4, 0.3))
    n = 20000
    for h, w in ((2, 2), (6, 6), (12, 24), (24, 24), (33, 6)):
        rows = so.draw_resize(n, h, w, torch.Generator().manual_seed(h + w)).numpy()
        assert rows.shape == (n, 8) and rows.dtype == np.int32 and not rows[:, 2:6].any() and not rows[:, 7].any()
        assert all(refs.size_ok(hi, wi, h, w) for hi, wi in set(map(tuple, rows[:, :2].tolist())))
        keep = (rows[:, 0] == 0) & (rows[:, 1] == 0)
        assert not rows[keep, 6].any() and (rows[~keep, :2] > 0).all()
        margin = 5 * math.sqrt(0.25 / n)                                               # five standard deviations of a frequency
        up, down = (rows[:, 0] >= h) & ~keep, (rows[:, 0] < h) & ~keep                 # s >= 1 gives hi >= h, s < 1 gives hi < h
        assert abs(keep.mean() - 0.3) < margin and abs(up.mean() - 0.3) < margin and abs(down.mean() - 0.4) < margin
        assert rows[~keep, 0].max() <= int(h * 1.2) and rows[~keep, 0].min() >= max(int(h * 0.3), -(-h // 4))
        m1, m2 = rows[~keep, 6] & 3, rows[~keep, 6] >> 2
        for m in (m1, m2):
            assert set(m.tolist()) == set(RESIZE_MODES.values())
            assert all(abs((m == v).mean() - 1 / 3) < 5 * math.sqrt(0.25 / (~keep).sum()) for v in range(3))
        assert abs(((m1 == m2).mean()) - 1 / 3) < 5 * math.sqrt(0.25 / (~keep).sum())   # drawn independently
    # the same s on both axes
    rows = so.draw_resize(2000, 24, 12, torch.Generator().manual_seed(1)).numpy()
    sized = rows[rows[:, 0] > 0]
    assert (np.abs(sized[:, 0] - 2 * sized[:, 1]) <= 2).all()
    assert np.array_equal(rows, so.draw_resize(2000, 24, 12, torch.Generator().manual_seed(1)).numpy())
    one_mode = SecondOrder(resize_prob=(0.0, 1.0, 0.0), resize_range=(0.5, 1.0), resize_modes=("bilinear",)).draw_resize(50, 24, 24).numpy()
    assert (one_mode[:, 6] == (1 | 1 << 2)).all() and (one_mode[:, 0] >= 12).all() and (one_mode[:, 0] <= 24).all()
    for kw, match in ((dict(resize_prob=(0.5, 0.6, 0.1)), "sum to 1"), (dict(resize_prob=(0.5, 0.5)), "sum to 1"),
                      (dict(resize_prob=(1, 0, 0), resize_range=(0.3, 2.5)), "resize_range"),
                      (dict(resize_prob=(1, 0, 0), resize_range=(1.1, 1.2)), "resize_range"),
                      (dict(resize_prob=(1, 0, 0), resize_modes=("nearest",)), "resize_modes")):
        with pytest.raises(ValueError, match=match):
            SecondOrder(**kw)
    with pytest.raises(ValueError, match="no resize"):
        SecondOrder().draw_resize(4, 24, 24)


def test_resize_off_draws_as_before_and_on_moves_the_noise():
    from srganst.device_data import SecondOrder
    kw = dict(ksize=7, bank_size=24, sinc_bank_size=8)
    plain, off, on = SecondOrder(**kw), SecondOrder(**kw, resize_prob=None), SecondOrder(**kw, resize_prob=(0.3, 0.4, 0.3))
    assert not plain.has_resize and not off.has_resize and on.has_resize and repr(off) == repr(plain) and "resize_prob" in repr(on)
    g = lambda: torch.Generator().manual_seed(9)
    want = plain.draw(64, g()).numpy()
    assert np.array_equal(off.draw(64, g()).numpy(), want) and np.array_equal(off.draw_bank(g()), plain.draw_bank(g()))
    assert np.array_equal(on.draw_bank(g()), plain.draw_bank(g()))
    got = on.draw(64, g()).numpy()
    assert np.array_equal(got[1:], want[1:]) and not got[0, :, 1:4].any() and want[0, :, 1:3].any()
    assert np.array_equal(got[0][:, [0, 4, 5, 6, 7]], want[0][:, [0, 4, 5, 6, 7]])
    assert np.array_equal(on.draw(64, g(), keep_noise=True).numpy(), want)
    # the noise words land in the resize rows; a sample that keeps its size, has a blur and no noise still gets its rounding from R
    r = on.draw_resize(64, 12, 12, g(), noise=want[0]).numpy()
    bare = on.draw_resize(64, 12, 12, g()).numpy()
    assert np.array_equal(r[:, 2:4], want[0][:, 1:3]) and np.array_equal(r[:, 4:6], want[0][:, 4:6])
    assert np.array_equal(r[:, 6] >> 4, want[0][:, 3]) and np.array_equal(r[:, 6] & 15, bare[:, 6]) and np.array_equal(r[:, :2], bare[:, :2])
    quiet = want[0].copy()
    quiet[:, 1:4] = 0
    r = on.draw_resize(64, 12, 12, g(), noise=quiet).numpy()
    kept, blurred = bare[:, 0] == 0, quiet[:, 0] >= 0
    assert (kept & blurred).any() and (kept & ~blurred).any()
    assert (r[kept & blurred, :2] == 12).all() and not r[kept & blurred, 6].any() and not r[kept & ~blurred, :2].any()
    # fixed
    fx = SecondOrder.fixed(noise=5.0, shot=0.01, gray=True, key=77, resize=(0.77, "bicubic", "area"))
    assert fx.has_resize and not SecondOrder.fixed(noise=5.0).has_resize and "resize=(0.77, 'bicubic', 'area')" in repr(fx)
    a = fx.draw(3).numpy()
    full = fx.draw(3, keep_noise=True).numpy()
    assert not a[0, :, 1:4].any() and np.array_equal(full, SecondOrder.fixed(noise=5.0, shot=0.01, gray=True, key=77).draw(3).numpy())
    r = fx.draw_resize(3, 33, 40, noise=full[0]).numpy()
    assert (r[:, 0] == 25).all() and (r[:, 1] == 30).all() and (r[:, 6] == (2 | 0 << 2 | 16)).all()
    assert np.array_equal(r[:, 2:4], full[0][:, 1:3]) and (r[:, 4] == 77).all()
    assert SecondOrder.fixed(resize=(0.25, "area", "area")).draw_resize(1, 33, 2).numpy()[0, :2].tolist() == [9, 1]
    for bad in ((0.2, "area", "area"), (2.5, "area", "area"), (1.0, "nearest", "area"), (1.0, "area")):
        with pytest.raises(ValueError, match="resize"):
            SecondOrder.fixed(resize=bad)


def test_loader_draws_per_tile_with_resize(monkeypatch):
    """A tile's resize row in an epoch depends on neither world size, rank nor batch size; every other draw is the one made without it;
    with resize off the loader draws what it drew before, from the generators it made before."""
    from torch.utils.data.distributed import DistributedSampler
    from srganst.device_data import Degradation, DeviceCropLoader, SecondOrder
    arena = _ArenaLR([(60, 70), (40, 90), (33, 35)], 16, 8, out=8)
    kw = dict(ksize=7, bank_size=24, sinc_bank_size=8)
    deg, so, so_r = Degradation(jpeg_prob=0.5), SecondOrder(**kw), SecondOrder(**kw, resize_prob=(0.3, 0.4, 0.3))
    base = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg, second=so)
    on = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg, second=so_r)
    assert base.resize_draws(0) is None and DeviceCropLoader(arena, 2, None, seed=3, degradation=deg).resize_draws(0) is None
    for epoch in (0, 1, 5):
        assert np.array_equal(on.draws(epoch), base.draws(epoch)) and np.array_equal(on.deg_draws(epoch), base.deg_draws(epoch))
        (rows, bank), (rows0, bank0) = on.second_draws(epoch), base.second_draws(epoch)
        assert np.array_equal(bank, bank0) and np.array_equal(rows[1:], rows0[1:]) and not rows[0, :, 1:4].any()
        assert np.array_equal(rows[0][:, [0, 4, 5]], rows0[0][:, [0, 4, 5]])
        r = on.resize_draws(epoch)
        assert r.shape == (len(arena), 8) and np.array_equal(r, on.resize_draws(epoch))
        assert np.array_equal(r[:, 2:4], rows0[0][:, 1:3]) and np.array_equal(r[:, 4:6], rows0[0][:, 4:6])
        assert np.array_equal(r[:, 6] >> 4, rows0[0][:, 3]) and all(refs.size_ok(hi, wi, 8, 8) for hi, wi in r[:, :2].tolist())
    assert not np.array_equal(on.resize_draws(0)[:, :2], on.resize_draws(1)[:, :2])
    other = DeviceCropLoader(arena, 2, None, True, True, seed=4, degradation=deg, second=so_r)
    assert not np.array_equal(on.resize_draws(0)[:, :2], other.resize_draws(0)[:, :2])
    all1, by_tile = on.resize_draws(1), {}
    for world in (1, 2, 4):
        for batch in (2, 5):
            for rank in range(world):
                sampler = DistributedSampler(arena, world, rank, shuffle=True, seed=11)
                sampler.set_epoch(1)
                ld = DeviceCropLoader(arena, batch, sampler, True, True, seed=3, degradation=deg, second=so_r)
                ld.set_epoch(1)
                order = np.fromiter(iter(sampler), dtype=np.int64)[: len(ld) * batch]
                desc, rows, rows2, bank, resize = ld.plan_resize()
                assert np.array_equal(desc.numpy(), base.draws(1)[order]) and np.array_equal(rows.numpy(), base.deg_draws(1)[order])
                assert tuple(resize.shape) == (len(order), 8) and resize.is_contiguous() and resize.dtype == torch.int32
                assert np.array_equal(rows2.numpy(), on.second_draws(1)[0][:, order]) and len(ld.plan_all()) == 4
                for i, tile in enumerate(order.tolist()):
                    r = resize[i].numpy()
                    assert np.array_equal(by_tile.setdefault(tile, r), r) and np.array_equal(r, all1[tile])
    assert len(by_tile) == len(arena)
    # resize off: the generators of before (the sampler's, window / transform, first stage, second stage, bank) and a fifth tuple slot
    made = []
    real = torch.Generator
    monkeypatch.setattr(torch, "Generator", lambda *a, **k: (made.append(1), real(*a, **k))[1])
    assert base.plan_resize()[4] is None and len(made) == 5
    made.clear()
    assert on.plan_resize()[4] is not None and len(made) == 7                    # + the third generator again, and the fourth


def test_config_switches():
    from srganst.config import Config
    from srganst.device_data import SecondOrder, check_switches
    cfg = Config()
    d = cfg.DATA
    assert d.DEGRADE2_RESIZE is False and d.VALIDATE_DEGRADE_RESIZE is None
    assert (d.DEGRADE2_RESIZE_PROB, d.DEGRADE2_RESIZE_RANGE, d.DEGRADE2_RESIZE_MODES) == ((0.3, 0.4, 0.3), (0.3, 1.2), ("area", "bilinear", "bicubic"))
    d.ON_DEVICE_WHOLE_IMAGES = d.DEGRADE = True
    d.DEGRADE2_RESIZE = True
    with pytest.raises(ValueError, match="DEGRADE2_RESIZE needs DATA.DEGRADE_SECOND"):
        check_switches(cfg)
    d.DEGRADE_SECOND = True
    check_switches(cfg)
    so = SecondOrder.from_config(cfg)
    assert so.has_resize and so.resize_prob == (0.3, 0.4, 0.3) and so.resize_range == (0.3, 1.2) and so.resize_modes == ("area", "bilinear", "bicubic")
    d.DEGRADE2_RESIZE_PROB, d.DEGRADE2_RESIZE_RANGE, d.DEGRADE2_RESIZE_MODES = (0.5, 0.5, 0.0), (0.5, 1.5), ("bicubic",)
    so = SecondOrder.from_config(cfg)
    assert (so.resize_prob, so.resize_range, so.resize_modes) == ((0.5, 0.5, 0.0), (0.5, 1.5), ("bicubic",))
    d.DEGRADE2_RESIZE = False
    off = SecondOrder.from_config(cfg)
    assert not off.has_resize and off.resize_prob is None
    g = lambda: torch.Generator().manual_seed(2)
    assert np.array_equal(off.draw(16, g()).numpy(), SecondOrder().draw(16, g()).numpy())


def test_validation_parameter():
    from srganst.config import Config
    from srganst.validate import _resize_param
    cfg = Config()
    assert _resize_param(cfg, None) is None and _resize_param(cfg, 0.5) == 0.5
    cfg.DATA.VALIDATE_DEGRADE_RESIZE = 1.5
    assert _resize_param(cfg, None) == 1.5 and _resize_param(cfg, 0.25) == 0.25
    for bad in (0.2, 2.5, -1):
        with pytest.raises(ValueError, match="VALIDATE_DEGRADE_RESIZE"):
            _resize_param(cfg, bad)
