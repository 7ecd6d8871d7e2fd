"""CPU: the fp64 restatement of the first stage's random resize (tests/resize1_refs.py) against F.interpolate, its bound's ingredients,
Degradation(resize_prob=...) and draw_resize, the loader's fifth generator, the config switches and validation's parameter."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize1_refs as refs
from test_filter_refs import _ArenaLR

TORCH_MODE = {0: "area", 1: "bilinear", 2: "bicubic"}
up8 = lambda n: -(-n // 8)


# ---- the restatement
@pytest.mark.parametrize("H, h", [(8, 2), (12, 3), (20, 5), (36, 9), (50, 12)])
def test_axis_matrices_against_torch_in_fp64(H, h):
    """Every intermediate size from ceil(H / 8) to 2 H, the three modes, H -> hi and hi -> h (area down-samples with up to 9 and up to
    2 H / h + 1 taps among them): within 1e-12 of F.interpolate(size=...) in fp64."""
    g = torch.Generator().manual_seed(H * 100 + h)
    W, w = H + 4, h + 1                                   # the other axis at a ratio of its own, within the same limits
    x = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    worst, most = 0.0, 0
    for hi in range(up8(H), 2 * H + 1):
        wi = min(max(int(W * hi / H), up8(W)), 2 * W)
        for mode in (0, 1, 2):
            kw = {} if mode == 0 else {"align_corners": False}
            want = F.interpolate(x, size=(hi, wi), mode=TORCH_MODE[mode], **kw)
            worst = max(worst, float(np.abs(refs.resize(x[0].numpy(), (hi, wi), mode) - want[0].numpy()).max()))
            down = F.interpolate(want, size=(h, w), mode=TORCH_MODE[mode], **kw)
            worst = max(worst, float(np.abs(refs.resize(want[0].numpy(), (h, w), mode) - down[0].numpy()).max()))
        most = max(most, refs.taps(0, H, hi), refs.taps(0, hi, h))
    print(f"axis matrices {H} -> .. -> {h}: max |restatement - F.interpolate| = {worst:.3g}, area taps up to {most}")
    assert worst <= 1e-12
    assert most > 5                                      # beyond section 24's fixed table


def test_tap_counts_are_the_matrices_and_stay_within_the_kernel_s_limits():
    for H, h in ((8, 2), (12, 3), (50, 12), (96, 24), (64, 4)):
        for hi in (up8(H), max(int(0.15 * H), up8(H)), int(0.77 * H), H, 2 * H):
            for n_in, n_out in ((H, hi), (hi, h)):
                for mode in (0, 1, 2):
                    M = refs.axis_matrix(mode, n_in, n_out)
                    assert np.allclose(M.sum(1), 1.0, atol=1e-14)
                    assert int((M != 0).sum(1).max()) <= refs.taps(mode, n_in, n_out)
            assert refs.taps(0, H, hi) <= 9 and refs.taps(0, hi, h) <= 2 * H // h + 1
    assert refs.taps(0, 96, 12) == 8 and refs.taps(0, 100, 13) == 9 and refs.taps(0, 128, 4) == 32 and refs.taps(0, 127, 4) == 33


def test_bound_grows_with_what_it_models():
    from srganst.device_data import rescale_rows
    row = lambda size, m, nz=0.0, sp=0.0: rescale_rows([size], m, nz, sp, 0, [(1, 2)])[0]
    b = lambda r, g=(96, 96, 24, 24): refs.row_bound(r, *g)
    aa, bb, cc = ("area", "area"), ("bilinear", "bilinear"), ("bicubic", "bicubic")
    assert 0 < b(row((48, 48), aa)) < b(row((48, 48), cc)) and b(row((48, 48), bb)) < b(row((48, 48), cc))
    assert b(row((144, 144), aa)) > b(row((48, 48), aa))                          # 7 taps on the way down against 3
    assert b(row((48, 48), cc, 10.0)) > b(row((48, 48), cc)) and b(row((48, 48), cc, 10.0, 0.01)) > b(row((48, 48), cc, 10.0))
    assert b(row(None, aa)) > 0                                                    # keep still resizes (96 -> 24)
    assert b(row(None, aa), (24, 24, 24, 24)) == 0                                 # equal geometry: the pass-through
    # the actual counts: 96 -> 12 (8 taps) -> 24 (1 tap), area both ways, no noise; section 24's formula by hand
    u, E, V = refs.U, 0.0, 1.0
    for T in (8, 8, 1, 1):
        E = E + T * 0.5 * u * V + T * u * V
    assert b(row((12, 12), aa)) == pytest.approx(E, rel=1e-12)
    assert b(row((48, 48), cc)) < 2e-4 and b(row((144, 144), ("bicubic", "area"))) < 1e-4


def test_reference_conventions():
    from srganst.device_data import rescale_rows
    x = np.random.default_rng(0).random((2, 3, 16, 24)).astype(np.float32)
    rows = rescale_rows([None, (1, 3)], ("area", "bilinear"), 0.0, 0.0, 0, [(1, 2), (3, 4)])
    out = refs.rescale_to_reference(x, rows, (4, 6), quantise=False)
    assert np.isnan(out[1]).all()                                                  # 8 * 1 < 16
    want = x[0].astype(np.float64).reshape(3, 4, 4, 6, 4).mean((2, 4))             # keep + area = the 4 x 4 block means
    want_b = refs.resize(x[0].astype(np.float64), (4, 6), 1)
    assert np.allclose(out[0], want_b, atol=1e-15) and not np.allclose(out[0], want)
    rows[0, 6] = 0 | 0 << 2
    assert np.allclose(refs.rescale_to_reference(x, rows, (4, 6), quantise=False)[0], want, atol=1e-15)
    same = refs.rescale_to_reference(x, rows, (16, 24), quantise=True)
    assert np.array_equal(same[0], x[0].astype(np.float64))                        # equal geometry, no size, no noise: the bits


# ---- Degradation(resize_prob=...) and draw_resize
def _deg(**kw):
    from srganst.device_data import Degradation
    return Degradation(**kw)


def test_draw_resize_sizes_kinds_and_modes():
    from srganst.device_data import RESIZE_MODES, Degradation, resize1_size
    prob = (0.2, 0.7, 0.1)
    d = _deg(resize_prob=prob)
    assert d.has_resize and not _deg().has_resize
    for H in (8, 12, 24, 33, 96):
        W = H + 3
        g = torch.Generator().manual_seed(H)
        deg = d.draw(4000, torch.Generator().manual_seed(H + 1)).numpy()
        r = d.draw_resize(4000, H, W, g, deg_rows=deg).numpy()
        assert r.dtype == np.int32 and r.shape == (4000, 8)
        assert all(refs.size_ok(hi, wi, H, W) for hi, wi in r[:, :2].tolist())
        keep = r[:, 0] == 0
        assert keep.any() and (r[keep, 1] == 0).all() and ((r[:, 0] == 0) == (r[:, 1] == 0)).all()
        assert (r[~keep, 0] >= up8(H)).all() and (r[~keep, 0] <= int(1.5 * H)).all()
        assert (r[~keep, 0] == up8(H)).any() or H >= 24                            # int(0.15 H) raised to the limit
        # the same s on both axes: some s in the range gives both sizes
        for hi, wi in r[~keep, :2][:200].tolist():
            lo = max((hi if hi > up8(H) else 0) / H, (wi if wi > up8(W) else 0) / W)
            top = min((hi + 1) / H, (wi + 1) / W)
            assert lo < top, (H, hi, wi)
        assert np.array_equal(r[:, 2], deg[:, 3]) and np.array_equal(r[:, 4:6], deg[:, 4:6])      # sigma_n and the key: the deg rows'
        assert not r[:, 3].any() and not (r[:, 6] >> 4).any() and not r[:, 7].any()                # shot = 0, gray = 0
        assert (r[keep, 6] & 3 == 0).all() and len(set((r[keep, 6] >> 2).tolist())) == 3            # keep still draws m2
    n = 20000
    r = d.draw_resize(n, 96, 96, torch.Generator().manual_seed(7)).numpy()
    assert not r[:, 2:6].any()                                                     # without deg_rows: no noise, no key
    keep = r[:, 0] == 0
    down = ~keep & (r[:, 0] <= 96)
    up = ~keep & ~down
    # (an up-sample at s < 1 + 1/96 lands on 96 and counts as down: 0.2 * (1/96) / 0.5 of the draws)
    shift = prob[0] * (1 / 96) / 0.5
    for got, p in ((up.mean(), prob[0] - shift), (down.mean(), prob[1] + shift), (keep.mean(), prob[2])):
        assert abs(got - p) <= 5 * math.sqrt(p * (1 - p) / n), (got, p)
    for shift_bits, sel in ((0, ~keep), (2, np.ones(n, bool))):
        m = (r[sel, 6] >> shift_bits) & 3
        for code in RESIZE_MODES.values():
            assert abs((m == code).mean() - 1 / 3) <= 5 * math.sqrt((2 / 9) / sel.sum()), (shift_bits, code)
    m1, m2 = r[~keep, 6] & 3, (r[~keep, 6] >> 2) & 3
    assert abs(np.mean(m1 == m2) - 1 / 3) <= 5 * math.sqrt((2 / 9) / (~keep).sum())               # drawn independently
    assert np.array_equal(r, d.draw_resize(n, 96, 96, torch.Generator().manual_seed(7)).numpy())
    one = _deg(resize_prob=(0.0, 1.0, 0.0), resize_range=(0.15, 1.0), resize_modes=("bilinear",))
    r = one.draw_resize(500, 96, 96, torch.Generator().manual_seed(1)).numpy()
    assert (r[:, 6] == (1 | 1 << 2)).all() and (r[:, 0] >= 14).all() and (r[:, 0] <= 96).all() and (r[:, 0] == r[:, 1]).all()
    assert resize1_size(96, 0.15) == 14 and resize1_size(8, 0.15) == 1 and resize1_size(33, 0.15) == 5 and resize1_size(33, 1.5) == 49
    f = Degradation.fixed(1.0, 2.0, 30.0, 5.0, key=9, resize=(0.77, "area", "bicubic"))
    assert f.has_resize and not Degradation.fixed(1.0, 2.0, 30.0, 5.0).has_resize
    rows = f.draw(3).numpy()
    r = f.draw_resize(3, 50, 70, deg_rows=rows).numpy()
    assert (r[:, 0] == 38).all() and (r[:, 1] == 53).all() and (r[:, 6] == (0 | 2 << 2)).all()
    assert np.array_equal(r[:, 2], rows[:, 3]) and np.array_equal(r[:, 4:6], rows[:, 4:6])
    assert "resize=(0.77, 'area', 'bicubic')" in repr(f)
    with pytest.raises(ValueError, match="this stage has no resize"):
        _deg().draw_resize(2, 8, 8)
    for bad in ((0.1, "area", "area"), (2.5, "area", "area"), (1.0, "nearest", "area"), (1.0, "area")):
        with pytest.raises(ValueError, match="Degradation.fixed: resize"):
            Degradation.fixed(1.0, 1.0, 0.0, 0.0, resize=bad)
    for kw, msg in ((dict(resize_prob=(0.5, 0.6, 0.1)), "three probabilities"), (dict(resize_prob=(0.5, 0.5)), "three probabilities"),
                    (dict(resize_range=(0.0, 1.5)), "resize_range"), (dict(resize_range=(0.5, 2.5)), "resize_range"),
                    (dict(resize_range=(1.2, 1.5)), "resize_range"), (dict(resize_modes=("nearest",)), "resize_modes"),
                    (dict(resize_modes=()), "resize_modes")):
        with pytest.raises(ValueError, match=msg):
            _deg(**kw)


def test_resize_off_is_the_instance_built_without_the_arguments():
    from srganst.device_data import Degradation
    for kw in (dict(), dict(jpeg_prob=0.5, blur_prob=0.7, aniso=False)):
        a, b = Degradation(**kw), Degradation(**kw, resize_prob=None, resize_range=(0.5, 1.2), resize_modes=("area",))
        assert repr(a) == repr(b) and "resize" not in repr(a) and not b.has_resize
        g = lambda: torch.Generator().manual_seed(5)
        assert np.array_equal(a.draw(64, g()).numpy(), b.draw(64, g()).numpy())
        on = Degradation(**kw, resize_prob=(0.2, 0.7, 0.1))
        assert np.array_equal(a.draw(64, g()).numpy(), on.draw(64, g()).numpy())   # draw() itself never changes
        assert repr(on) == repr(a)[:-1] + (", resize_prob=(0.2, 0.7, 0.1), resize_range=(0.15, 1.5), "
                                           "resize_modes=('area', 'bilinear', 'bicubic'))")
    f = Degradation.fixed(1.0, 2.0, 30.0, 5.0, key=9, jpeg=40)
    assert repr(f) == repr(Degradation.fixed(1.0, 2.0, 30.0, 5.0, key=9, jpeg=40, resize=None)) and "resize" not in repr(f)


# ---- the loader's fifth generator
def test_loader_draws_per_tile_with_the_first_stage_resize(monkeypatch):
    """A tile's first-stage resize row in an epoch depends on neither world size, rank nor batch size; every other draw is the one made
    without it; with the option off the loader draws what it drew before, from the generators it made before."""
    from torch.utils.data.distributed import DistributedSampler
    from srganst.device_data import Degradation, DeviceCropLoader, SecondOrder
    arena = _ArenaLR([(60, 70), (40, 90), (33, 35)], 16, 8, out=4)
    kw = dict(ksize=7, bank_size=24, sinc_bank_size=8, resize_prob=(0.3, 0.4, 0.3))
    deg, deg_r, so = Degradation(jpeg_prob=0.5, ksize=7), Degradation(jpeg_prob=0.5, ksize=7, resize_prob=(0.2, 0.7, 0.1)), SecondOrder(**kw)
    base = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg, second=None)
    on = DeviceCropLoader(arena, 2, None, True, True, seed=3, degradation=deg_r, second=None)
    assert base.resize1_draws(0) is None and DeviceCropLoader(arena, 2, None, seed=3).resize1_draws(0) is None
    for epoch in (0, 1, 5):
        assert np.array_equal(on.draws(epoch), base.draws(epoch)) and np.array_equal(on.deg_draws(epoch), base.deg_draws(epoch))
        r = on.resize1_draws(epoch)
        d = base.deg_draws(epoch)
        assert r.shape == (len(arena), 8) and np.array_equal(r, on.resize1_draws(epoch))
        assert np.array_equal(r[:, 2], d[:, 3]) and np.array_equal(r[:, 4:6], d[:, 4:6]) and not r[:, 3].any()
        assert all(refs.size_ok(hi, wi, 16, 16) for hi, wi in r[:, :2].tolist())
    assert not np.array_equal(on.resize1_draws(0)[:, :2], on.resize1_draws(1)[:, :2])
    other = DeviceCropLoader(arena, 2, None, True, True, seed=4, degradation=deg_r)
    assert not np.array_equal(on.resize1_draws(0)[:, :2], other.resize1_draws(0)[:, :2])
    # with the second stage and its own resize beside it: their draws are the ones made without the first stage's
    arena2 = _ArenaLR([(60, 70), (40, 90), (33, 35)], 16, 8, out=8)
    base2 = DeviceCropLoader(arena2, 2, None, True, True, seed=3, degradation=deg, second=so)
    on2 = DeviceCropLoader(arena2, 2, None, True, True, seed=3, degradation=deg_r, second=so)
    for epoch in (0, 2):
        assert np.array_equal(on2.second_draws(epoch)[0], base2.second_draws(epoch)[0])
        assert np.array_equal(on2.second_draws(epoch)[1], base2.second_draws(epoch)[1])
        assert np.array_equal(on2.resize_draws(epoch), base2.resize_draws(epoch))
        assert np.array_equal(on2.resize1_draws(epoch), on.resize1_draws(epoch))   # and it does not see the second stage
    all1, by_tile = on2.resize1_draws(1), {}
    for world in (1, 2, 4):
        for batch in (2, 5):
            for rank in range(world):
                sampler = DistributedSampler(arena2, world, rank, shuffle=True, seed=11)
                sampler.set_epoch(1)
                ld = DeviceCropLoader(arena2, batch, sampler, True, True, seed=3, degradation=deg_r, second=so)
                ld.set_epoch(1)
                order = np.fromiter(iter(sampler), dtype=np.int64)[: len(ld) * batch]
                desc, rows, rows2, bank, resize, first = ld.plan_first_resize()
                assert np.array_equal(desc.numpy(), base2.draws(1)[order]) and np.array_equal(rows.numpy(), base2.deg_draws(1)[order])
                assert np.array_equal(rows2.numpy(), base2.second_draws(1)[0][:, order])
                assert np.array_equal(resize.numpy(), base2.resize_draws(1)[order])
                assert tuple(first.shape) == (len(order), 8) and first.is_contiguous() and first.dtype == torch.int32
                assert len(ld.plan_resize()) == 5 and len(ld.plan_all()) == 4
                for i, tile in enumerate(order.tolist()):
                    r = first[i].numpy()
                    assert np.array_equal(by_tile.setdefault(tile, r), r) and np.array_equal(r, all1[tile])
    assert len(by_tile) == len(arena2)
    # the option off: the generators of before (sampler, window / transform, first stage), and a sixth tuple slot that is None
    made = []
    real = torch.Generator
    monkeypatch.setattr(torch, "Generator", lambda *a, **k: (made.append(1), real(*a, **k))[1])
    assert base.plan_first_resize()[5] is None and len(made) == 3
    made.clear()
    assert on.plan_first_resize()[5] is not None and len(made) == 5                # + the second generator again, and the fifth


def test_config_switches(capsys):
    from srganst.config import Config
    from srganst.device_data import Degradation, announce_degradation, check_switches
    cfg = Config()
    d = cfg.DATA
    assert d.DEGRADE_RESIZE is False and d.VALIDATE_DEGRADE_RESIZE1 is None
    assert (d.DEGRADE_RESIZE_PROB, d.DEGRADE_RESIZE_RANGE, d.DEGRADE_RESIZE_MODES) == ((0.2, 0.7, 0.1), (0.15, 1.5), ("area", "bilinear", "bicubic"))
    d.ON_DEVICE_WHOLE_IMAGES = True
    d.DEGRADE_RESIZE = True
    with pytest.raises(ValueError, match="DATA.DEGRADE_RESIZE needs DATA.DEGRADE = True: the first stage's random resize"):
        check_switches(cfg)
    d.DEGRADE = True
    check_switches(cfg)
    deg = Degradation.from_config(cfg)
    assert deg.has_resize and (deg.resize_prob, deg.resize_range, deg.resize_modes) == ((0.2, 0.7, 0.1), (0.15, 1.5), ("area", "bilinear", "bicubic"))
    d.DEGRADE_RESIZE_PROB, d.DEGRADE_RESIZE_RANGE, d.DEGRADE_RESIZE_MODES = (0.5, 0.5, 0.0), (0.5, 1.2), ("bicubic",)
    deg = Degradation.from_config(cfg)
    assert (deg.resize_prob, deg.resize_range, deg.resize_modes) == ((0.5, 0.5, 0.0), (0.5, 1.2), ("bicubic",))
    announce_degradation(cfg, deg)
    out = capsys.readouterr().out
    assert out.count("\n") == 2 and out.count("[Data] DATA.DEGRADE_RESIZE: instead lr = ") == 1
    assert "(up, down, keep) = (0.5, 0.5, 0.0), scale in (0.5, 1.2), modes ('bicubic',)" in out
    for key in ("DEGRADE_RESIZE_PROB", "DEGRADE_RESIZE_RANGE", "DEGRADE_RESIZE_MODES"):          # read with .get defaults
        del d[key]
    assert Degradation.from_config(cfg).resize_prob == (0.2, 0.7, 0.1)
    d.DEGRADE_RESIZE = False
    off = Degradation.from_config(cfg)
    assert not off.has_resize and off.resize_prob is None
    announce_degradation(cfg, off)
    assert "DEGRADE_RESIZE" not in capsys.readouterr().out
    g = lambda: torch.Generator().manual_seed(2)
    assert np.array_equal(off.draw(16, g()).numpy(), Degradation().draw(16, g()).numpy())
    del d["DEGRADE_RESIZE"]
    assert not Degradation.from_config(cfg).has_resize


def test_validation_parameter():
    from srganst.config import Config
    from srganst.validate import _resize1_param
    cfg = Config()
    assert _resize1_param(cfg, None) is None and _resize1_param(cfg, 0.5) == (0.5, "bicubic", "bicubic")
    assert _resize1_param(cfg, (0.5,)) == (0.5, "bicubic", "bicubic") and _resize1_param(cfg, (1.5, "area", "bilinear")) == (1.5, "area", "bilinear")
    cfg.DATA.VALIDATE_DEGRADE_RESIZE1 = (0.125, "bilinear", "area")
    assert _resize1_param(cfg, None) == (0.125, "bilinear", "area") and _resize1_param(cfg, 2)[0] == 2.0
    for bad in (0.1, 2.5, (0.5, "area"), (0.5, "nearest", "area"), ("x", "area", "area")):
        with pytest.raises(ValueError, match="VALIDATE_DEGRADE_RESIZE1"):
            _resize1_param(cfg, bad)
