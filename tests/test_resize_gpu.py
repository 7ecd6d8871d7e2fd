"""GPU: the resize round trip of the second-order degradation (csrc/resize.hip: sst_rescale; srganst.device_data: rescale,
second_order(resize_rows=...), SecondOrder(resize_prob=...), DeviceCropLoader; validate's degrade_resize) against the fp64 restatement
of tests/resize_refs.py and its derived bound."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import filter_refs
import resize_refs as refs
from test_degrade_gpu import _TwoPairs, _arena

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (7, 9), (24, 24), (33, 40), (65, 31)]
up4 = lambda n: -(-n // 4)


def _size(kind, h, w):
    if kind is None:
        return None
    return {"same": (h, w), "min": (up4(h), up4(w)), "max": (2 * h, 2 * w), "frac": (max(int(0.77 * h), up4(h)), max(int(0.77 * w), up4(w))),
            "aniso": (min(2 * h, h + max(1, h // 3)), max(up4(w), w - max(1, w // 3)))}[kind]


def _rows(spec, h, w):
    """[(size kind or None, m1, m2, noise255, shot, gray, key)] -> int32 [n, 8]."""
    from srganst.device_data import rescale_rows
    return torch.from_numpy(rescale_rows([_size(s[0], h, w) for s in spec], [(s[1], s[2]) for s in spec], [s[3] for s in spec],
                                         [s[4] for s in spec], [s[5] for s in spec], [(s[6], s[6] * 7919 + 1) for s in spec]))


# the row sets of the restatement cases, B = 1 and B = 3: pass-through, noise only, the image's own size, the smallest and the largest
# intermediate size, a non-integer ratio, an anisotropic pair (rows up, columns down), the nine mode pairs, colour, gray and shot noise
ROW_SETS = [
    [("frac", "bicubic", "bilinear", 10.0, 0.01, 1, 11)],
    [(None, "area", "area", 0.0, 0.0, 0, 1), (None, "area", "area", 20.0, 0.0, 0, 2), ("same", "bicubic", "bicubic", 20.0, 0.0, 0, 2)],
    [("min", "area", "area", 0.0, 0.0, 0, 3), ("max", "bilinear", "bilinear", 5.0, 0.0, 0, 4), ("frac", "bicubic", "area", 0.0, 0.02, 1, 5)],
    [("aniso", "area", "bilinear", 8.0, 0.01, 0, 6), ("frac", "area", "bicubic", 0.0, 0.0, 0, 7), ("max", "bilinear", "area", 3.0, 0.0, 1, 8)],
    [("min", "bilinear", "bicubic", 12.0, 0.0, 0, 9), ("aniso", "bicubic", "bilinear", 0.0, 0.0, 0, 10), ("max", "bicubic", "bicubic", 0.0, 0.0, 0, 12)],
]
assert {(s[1], s[2]) for rs in ROW_SETS for s in rs if s[0]} == {(a, b) for a in refs.MODES for b in refs.MODES}


@functools.lru_cache(maxsize=None)
def _input(B, h, w):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + B)
    return torch.rand(B, 3, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(h, w, which):
    """The unquantised fp64 restatement of one row set on the shared input: computed once, read by every test that needs it."""
    rows = _rows(ROW_SETS[which], h, w)
    ref = refs.rescale_reference(_input(len(rows), h, w).numpy(), rows.numpy(), quantise=False)
    ref.setflags(write=False)
    return ref


def _run(x, rows, **kw):
    from srganst.device_data import rescale
    return rescale(x.cuda(), rows.cuda(), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid(raw):
    return torch.round(255 * raw.clamp(0, 1)) / 255


@pytest.mark.parametrize("h, w", SHAPES)
def test_kernel_against_the_restatement(h, w):
    """Per sample: the unquantised output within the derived bound of the restatement; the quantised output = round(255 clamp(v)) / 255
    taken in fp32 from the unquantised launch; a pass-through sample keeps its bits."""
    worst, worst_abs = 0.0, 0.0
    for which, spec in enumerate(ROW_SETS):
        rows, x = _rows(spec, h, w), _input(len(spec), h, w)
        raw = _run(x, rows, quantise=False).cpu()
        ref, bound = _reference(h, w, which), refs.bound(rows.numpy())
        q = _run(x, rows).cpu()
        for b, s in enumerate(spec):
            if s[0] is None and s[3] == 0 and s[4] == 0:
                assert torch.equal(_bits(raw[b]), _bits(x[b])) and torch.equal(_bits(q[b]), _bits(x[b]))
                continue
            err = float(np.abs(raw[b].double().numpy() - ref[b]).max())
            worst, worst_abs = max(worst, err / bound[b]), max(worst_abs, err)
            print(f"rescale {h}x{w} rows {which}[{b}] {s[0]} {_size(s[0], h, w)} {s[1]}/{s[2]}: max |kernel - fp64| = {err:.3g}, "
                  f"bound {bound[b]:.3g}")
            assert err <= bound[b], (which, b, err, bound[b])
            assert torch.equal(q[b], _grid(raw[b])), (which, b)
            assert float(q[b].min()) >= 0 and float(q[b].max()) <= 1
    print(f"rescale {h}x{w}: worst error {worst_abs:.3g}, worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("h, w", [(7, 9), (33, 40)])
def test_the_image_s_own_size_and_no_size_are_the_filter_stage_s_noise(h, w):
    """On finite inputs the identity resize is exact and the Philox index coincides: (h, w) with noise = the 0, 0 row = sst_filter2d's
    noise-only output for the same key, bit for bit."""
    from srganst.device_data import filter2d, filter_rows
    x = _input(3, h, w)
    noise = [(20.0, 0.0, 0), (0.0, 0.02, 1), (6.0, 0.01, 0)]
    keys = [(5, 6), (7, 8), (9, 10)]
    flt = torch.from_numpy(filter_rows([-1] * 3, [n[0] for n in noise], [n[1] for n in noise], [n[2] for n in noise], keys))
    for quantise in (False, True):
        want = filter2d(x.cuda(), flt.cuda(), None, quantise=quantise)
        assert torch.equal(_run(x, _keyed(h, w, [(None, "area", "area", *n) for n in noise], keys), quantise=quantise), want)
        for m1, m2 in (("area", "bicubic"), ("bilinear", "area"), ("bicubic", "bilinear")):
            same = _run(x, _keyed(h, w, [("same", m1, m2, *n) for n in noise], keys), quantise=quantise)
            assert torch.equal(same, want), (m1, m2, quantise)


def _keyed(h, w, spec, keys):
    from srganst.device_data import rescale_rows
    return torch.from_numpy(rescale_rows([_size(s[0], h, w) for s in spec], [(s[1], s[2]) for s in spec], [s[3] for s in spec],
                                         [s[4] for s in spec], [s[5] for s in spec], keys))


def test_a_constant_image_comes_back():
    h, w = 33, 40
    x = torch.empty(3, 3, h, w)
    x[0], x[1], x[2] = 100 / 255, 1.0, 0.0
    for mode in refs.MODES:
        for kind in ("min", "frac", "max", "aniso"):
            rows = _rows([(kind, mode, mode, 0.0, 0.0, 0, 1)] * 3, h, w)
            assert torch.equal(_run(x, rows).cpu(), x), (mode, kind)
            raw = _run(x, rows, quantise=False).cpu()
            assert float((raw - x).abs().max()) <= refs.bound(rows.numpy()).max()


def test_pass_through_keeps_every_bit():
    h, w = 33, 40
    x = (_input(3, h, w) - 0.5) * 4
    x[0, 1, 3, 5], x[0, 2, 32, 39], x[2, 0, 0, 0], x[2, 1, 16, 20] = float("nan"), float("inf"), float("-inf"), float("nan")
    _bits(x)[0, 0, 0, 1] = 0x7FC01234                       # a NaN with a payload
    rows = _rows([(None, "area", "area", 0, 0, 0, 1), ("frac", "bilinear", "bilinear", 0, 0, 0, 2), (None, "bicubic", "bilinear", 0, 0, 1, 3)], h, w)
    for quantise in (True, False):
        out = _run(x, rows, quantise=quantise).cpu()
        assert torch.equal(_bits(out[0]), _bits(x[0])) and torch.equal(_bits(out[2]), _bits(x[2]))
        assert bool(torch.isfinite(out[1]).all()) and (not quantise or (float(out[1].min()) >= 0 and float(out[1].max()) <= 1))


def test_gray_noise_on_a_replicated_input_stays_replicated():
    h, w = 33, 40
    x = _input(1, h, w)[:, :1].expand(2, 3, h, w).contiguous()
    for kind in (None, "frac", "max"):
        spec = [(kind, "bicubic", "area", 20.0, 0.01, 1, 5), (kind, "bicubic", "area", 20.0, 0.01, 0, 5)]
        for quantise in (False, True):
            out = _run(x, _rows(spec, h, w), quantise=quantise)
            assert torch.equal(out[0, 0], out[0, 1]) and torch.equal(out[0, 0], out[0, 2])
            assert not torch.equal(out[1, 0], out[1, 1]) and not torch.equal(out[1, 1], out[1, 2])
            assert torch.equal(out[0, 0], out[1, 0])                              # e = Y * wi + X: channel 0's draws


def test_a_sample_sees_its_key_but_neither_its_position_the_batch_nor_the_tiles(monkeypatch):
    from srganst.device_data import rescale
    h, w = 65, 40
    spec = [("frac", "bicubic", "bilinear", 8.0, 0.0, 0, 1), (None, "area", "area", 0.0, 0.0, 0, 2), ("max", "area", "bicubic", 0.0, 0.02, 1, 3),
            ("min", "bilinear", "area", 12.0, 0.0, 0, 4), (None, "area", "area", 9.0, 0.01, 0, 5), ("aniso", "bicubic", "bicubic", 0.0, 0.0, 0, 6)]
    x, rows = _input(6, h, w).cuda(), _rows(spec, h, w).cuda()
    a = rescale(x, rows)
    assert torch.equal(rescale(x, rows), a)                                         # same inputs, same bits
    perm = torch.tensor([3, 0, 5, 4, 1, 2], device="cuda")
    assert torch.equal(rescale(x[perm].contiguous(), rows[perm].contiguous()), a[perm])
    for b in (0, 2, 3):
        assert torch.equal(rescale(x[b:b + 1].contiguous(), rows[b:b + 1].contiguous())[0], a[b])        # B = 1: other tile rows
    assert torch.equal(rescale(x[:3].contiguous(), rows[:3].contiguous()), a[:3])
    rekeyed = rows.clone()
    rekeyed[:, 4] += 1
    b = rescale(x, rekeyed)
    assert torch.equal(b[1], a[1]) and torch.equal(b[5], a[5]) and all(not torch.equal(b[i], a[i]) for i in (0, 2, 3, 4))
    raw = rescale(x, rows, quantise=False)
    for tile_rows in ("32", "8", "5", "1"):
        monkeypatch.setenv("SST_RESIZE_ROWS", tile_rows)
        assert torch.equal(rescale(x, rows), a) and torch.equal(rescale(x, rows, quantise=False), raw), tile_rows
    monkeypatch.delenv("SST_RESIZE_ROWS")
    # the forms: a new tensor (the input untouched), out=; out is x raises; a non-contiguous input is read as it is indexed; rows on
    # the host are checked and uploaded
    keep = x.clone()
    o = torch.full_like(x, 7.0)
    assert rescale(x, rows, out=o) is o and torch.equal(o, a) and torch.equal(x, keep)
    with pytest.raises(ValueError, match="out must not be x"):
        rescale(x, rows, out=x)
    wide = torch.zeros(6, 3, h, 50, device="cuda")
    wide[..., :w] = x
    assert torch.equal(rescale(wide[..., :w], rows), a)
    with pytest.raises(ValueError, match="out must be contiguous fp32"):
        rescale(x, rows, out=wide[..., :w])
    with pytest.raises(ValueError, match="deg must be contiguous int32"):
        rescale(x, rows[:4])
    with pytest.raises(ValueError, match="x must be fp32"):
        rescale(x.double(), rows)
    assert torch.equal(rescale(x, rows.cpu()), a)
    for hi, wi in ((up4(h) - 1, w), (h, 2 * w + 1), (0, w), (-1, -1)):
        bad = rows.cpu().clone()
        bad[2, 0], bad[2, 1] = hi, wi
        with pytest.raises(ValueError, match="row 2: the intermediate size"):
            rescale(x, bad)


def test_nan_conventions_touch_that_sample_only():
    from srganst.device_data import rescale
    h, w = 33, 40
    spec = [("frac", "bicubic", "area", 5.0, 0.0, 0, 1), ("max", "bilinear", "bicubic", 0.0, 0.01, 1, 2), (None, "area", "area", 0.0, 0.0, 0, 3)]
    x = _input(3, h, w).cuda()
    good = _rows(spec, h, w)
    clean = rescale(x, good.cuda())
    f32 = lambda v: int(np.float32(v).view(np.int32))
    sized, every = (0, 1), (0, 1, 2)
    cases = [(0, 0, sized), (1, 0, sized), (0, h, (2,)), (1, w, (2,)),                          # exactly one of hi, wi is zero
             (0, -3, every), (1, -3, every), (0, up4(h) - 1, sized), (1, up4(w) - 1, sized), (0, 2 * h + 1, sized), (1, 2 * w + 1, sized),
             (0, 1 << 30, sized), (0, -(1 << 31), sized),
             (6, 3, every), (6, 3 << 2, every), (6, 1 | 1 << 5, every), (6, 1 << 8, every), (6, -1, every), (6, -(1 << 31), every),
             (2, f32(-1e-3), every), (2, f32("nan"), every), (2, f32("-inf"), every), (3, f32(-1.0), every), (3, f32("nan"), every)]
    for word, value, victims in cases:
        for victim in victims:
            rows = good.clone()
            rows[victim, word] = value
            out = rescale(x, rows.cuda())
            assert bool(torch.isnan(out[victim]).all()), (word, value, victim)
            for other in set(range(3)) - {victim}:
                assert torch.equal(out[other], clean[other]), (word, value, victim, other)
    # a NaN pixel spreads over the taps that reach it and no further
    dirty = x.clone()
    dirty[2, 1, 16, 20] = float("nan")
    rows = good.clone()
    rows[2] = _rows([("same", "bilinear", "bilinear", 0.0, 0.0, 0, 3)], h, w)[0]
    base = rescale(x, rows.cuda())
    out = rescale(dirty, rows.cuda())
    mask = torch.zeros(3, h, w, dtype=torch.bool, device="cuda")
    mask[1, 14:17, 18:21] = True                         # a tap of weight 0 still carries it: rows 15, 16 of u, then 14..16 of y
    assert bool(torch.isnan(out[2, 1, 16, 20])) and torch.equal(out[2][~mask], base[2][~mask]) and torch.equal(out[:2], base[:2])


def test_captured_launch_replayed_on_fresh_data_and_rows():
    from srganst.device_data import rescale
    h, w = 33, 40
    spec = [("frac", "bicubic", "bilinear", 10.0, 0.0, 0, 1), (None, "area", "area", 0.0, 0.0, 0, 2), ("max", "area", "area", 0.0, 0.02, 1, 3)]
    x, rows = _input(3, h, w).cuda(), _rows(spec, h, w).cuda()
    want = rescale(x, rows)
    buf, out = x.clone(), torch.zeros_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, one kernel node
        rescale(buf, rows, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    fresh = (_input(3, h, w).flip(0) * 0.9).contiguous().cuda()
    fresh_rows = _rows([("min", "bilinear", "bicubic", 0.0, 0.0, 0, 7), ("aniso", "area", "bicubic", 3.0, 0.0, 1, 8),
                        (None, "area", "area", 4.0, 0.0, 0, 9)], h, w).cuda()
    buf.copy_(fresh), rows.copy_(fresh_rows)                                       # the graph reads both when it runs
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, rescale(fresh, fresh_rows))


def _second(ksize, **kw):
    from srganst.device_data import SecondOrder
    return SecondOrder(ksize=ksize, bank_size=24, sinc_bank_size=8, jpeg_quality=(20, 100), **kw)


@pytest.mark.parametrize("scale, ksize", [(2, 21), (4, 7)])                        # LR 12 x 12 under K = 21; LR 6 x 6 under K = 7
def test_loader_with_resize(scale, ksize, monkeypatch):
    """Two epochs over the small arena: lr is the public ops composed by hand (filter2d unquantised, rescale, filter2d, jpeg, filter2d)
    on the lr of the loader without the second stage; gt is that loader's; the last launch writes the bound buffer; an epoch repeats.
    With resize off: the bits of the loader as it was, and sst_rescale never launched."""
    from srganst import device_data
    from srganst.device_data import Degradation, DeviceCropLoader, filter2d, jpeg, rescale
    S, B = 24, 2
    o = S // scale
    _, arena, _, _ = _arena(S, scale)
    order = list(range(len(arena)))[::-1]
    first = Degradation(blur_prob=0.8, noise_prob=0.8, jpeg_prob=0.5, jpeg_chroma="444")
    kw = dict(jpeg_chroma="444", jpeg_prob=0.7, noise_prob=0.8)
    so, so_off = _second(ksize, resize_prob=(0.3, 0.4, 0.3), **kw), _second(ksize, **kw)
    on = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first, second=so)
    off2 = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first, second=so_off)
    off = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first)
    gt_buf, lr_buf = torch.zeros(B, 3, S, S, device="cuda"), torch.zeros(B, 3, o, o, device="cuda")
    seen, kinds = [], np.zeros(3, np.int64)
    for epoch in range(2):
        rows, bank = on.second_draws(epoch)
        resize = on.resize_draws(epoch)
        assert np.array_equal(bank, off2.second_draws(epoch)[1]) and np.array_equal(rows[1:], off2.second_draws(epoch)[0][1:])
        bank_d = torch.from_numpy(bank).cuda()
        if epoch == 1:
            on.bind(gt_buf, lr_buf)
        n = 0
        for (gt1, lr1), (gt0, lr0) in zip(on, off):
            sel = order[n * B:(n + 1) * B]
            r = torch.from_numpy(np.ascontiguousarray(rows[:, sel])).cuda()
            rr = torch.from_numpy(np.ascontiguousarray(resize[sel])).cuda()
            kinds += [(rr[:, 0] >= o).sum().item(),((rr[:, 0] < o) & (rr[:, 0] > 0)).sum().item(), (rr[:, 0] == 0).sum().item()]
            want = rescale(filter2d(lr0, r[0], bank_d, quantise=False), rr)
            want = filter2d(jpeg(filter2d(want, r[1], bank_d), r[2], "444"), r[3], bank_d)
            assert torch.equal(gt1, gt0) and torch.equal(lr1, want), (epoch, n)
            assert epoch == 0 or (lr1 is lr_buf and gt1 is gt_buf)
            assert torch.equal(lr1, device_data.second_order(lr0, r, bank_d, "444", resize_rows=rr))
            assert float(lr1.min()) >= 0 and float(lr1.max()) <= 1 and float((lr1 * 255 - torch.round(lr1 * 255)).abs().max()) < 1e-3
            seen.append(lr1.clone())
            n += 1
        assert n == len(on) >= 3
    assert (kinds > 0).all(), kinds                                                # up, down and keep each ran on some sample
    on.bind(None, None)
    on.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(seen, on))
    # resize off: the second stage's four launches and bits of before (filter2d, filter2d, jpeg, filter2d on its own rows)
    rows, bank = off2.second_draws(0)
    bank_d = torch.from_numpy(bank).cuda()
    before = []
    off.set_epoch(0)
    for n, (_, lr0) in enumerate(off):
        r = torch.from_numpy(np.ascontiguousarray(rows[:, order[n * B:(n + 1) * B]])).cuda()
        before.append(filter2d(jpeg(filter2d(filter2d(lr0, r[0], bank_d), r[1], bank_d), r[2], "444"), r[3], bank_d))

    def boom(*a, **k):
        raise AssertionError("sst_rescale launched by a loader without resize")
    monkeypatch.setattr(device_data, "rescale", boom)
    off2.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(before, off2))
    with pytest.raises(AssertionError, match="without resize"):
        on.set_epoch(0)
        list(on)


def test_loader_with_fixed_parameters_follows_the_restatement():
    """SecondOrder.fixed(resize=...) through the loader against the fp64 restatement, on the kernel's own blurred values."""
    from srganst import kernels
    from srganst.device_data import Degradation, DeviceCropLoader, SecondOrder, filter2d, rescale
    _, arena, _, _ = _arena(24, 2)
    order = list(range(len(arena)))
    table = kernels.plateau(21, 1.2, 0.7, 0.4, beta=1.3, support=9)
    first = Degradation.fixed(1.0, 2.0, 30.0, 3.0, key=5)
    off = DeviceCropLoader(arena, 4, order, degradation=first)
    for resize in ((0.77, "bicubic", "area"), (1.2, "bilinear", "bicubic"), (0.3, "area", "bilinear")):
        so = SecondOrder.fixed(kernel=table, noise=6.0, shot=0.004, gray=True, key=77, resize=resize)
        on = DeviceCropLoader(arena, 4, order, degradation=first, second=so)
        rows, bank = on.second_draws(0)
        rr = on.resize_draws(0)[:4]
        assert (rr[:, 0] == max(int(12 * resize[0]), 3)).all() and not rows[0, :, 1:4].any()
        (_, lr1), (_, lr0) = next(iter(on)), next(iter(off))
        a_raw = filter2d(lr0, torch.from_numpy(np.ascontiguousarray(rows[0, :4])).cuda(), torch.from_numpy(bank).cuda(), quantise=False)
        r_raw = rescale(a_raw, torch.from_numpy(np.ascontiguousarray(rr)).cuda(), quantise=False).cpu()
        ref = refs.rescale_reference(a_raw.cpu().numpy(), rr, quantise=False)
        bound = refs.bound(rr, xmax=float(a_raw.abs().max()))
        err = np.abs(r_raw.double().numpy() - ref).reshape(4, -1).max(1)
        assert (err <= bound).all(), (resize, err, bound)
        assert torch.equal(lr1.cpu(), _grid(r_raw))


def test_warmup_trains_on_resized_batches(tmp_path, monkeypatch, capsys):
    from srganst.config import Config
    from srganst.loss import MSELoss
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    _, arena, _, _ = _arena(24, 4)
    cfg = Config()
    cfg.EXP.NAME, cfg.EXP.N_EPOCHS, cfg.EXP.SAVE_STATE = "resize", 1, False
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    cfg.DATA.BATCH_SIZE, cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 2, 24, 8
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.LOG_TRAIN_PERIOD = 1
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = cfg.DATA.DEGRADE = cfg.DATA.DEGRADE_SECOND = True
    cfg.DATA.DEGRADE2_RESIZE = True
    cfg.DATA.DEGRADE2_KSIZE, cfg.DATA.DEGRADE2_BANK_SIZE, cfg.DATA.DEGRADE2_SINC_BANK_SIZE = 11, 16, 8        # LR 6 x 6: p = 5
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss()}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0}
    warmup(cfg, train_dataset=arena, test_dataset=_Pairs(), max_steps_per_epoch=3)
    out = capsys.readouterr().out
    assert out.count("DATA.DEGRADE_SECOND: then lr = ") == 1 and out.count("DATA.DEGRADE2_RESIZE: with lr * k2 unquantised") == 1
    assert "(up, down, keep) = (0.3, 0.4, 0.3), scale in (0.3, 1.2), modes ('area', 'bilinear', 'bicubic')" in out
    losses = [float(v) for m in re.findall(r"\[G losses: \{([^}]*)\}", out) for v in re.findall(r": ([-+0-9.einfa]+)", m)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    assert os.path.exists("results/resize/g_last.pth")


def test_validation_with_degrade_resize(tmp_path, capsys):
    """Both validation paths, whole and tiled: the input is the resize round trip of degrade(gt) (or of the plain bicubic LR made from
    gt), before the sinc and JPEG stages; the head line names the scale; off: the numbers of before."""
    from torch.utils.data import DataLoader
    from srganst import kernels
    from srganst.config import Config
    from srganst.device_data import Degradation, DeviceTestSet, degrade, filter2d, filter_rows, jpeg, rescale, rescale_rows
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    cfg.EXP.NAME = "val"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    ds = _TwoPairs()
    params, omega, s = (0.6, 3.5, 30.0, 10.0), 1.5, 0.7
    bank = torch.from_numpy(kernels.bank([kernels.sinc(21, omega)])).cuda()
    flt = torch.from_numpy(filter_rows([0], 0, 0, 0, [(0, 0)])).cuda()
    q40 = torch.zeros(1, 8, dtype=torch.int32, device="cuda")
    q40[0, 6] = 40

    def trip(t):
        h, w = t.shape[2:]
        rows = rescale_rows([(int(h * s), int(w * s))], ("bicubic", "bicubic"), 0, 0, 0, [(0, 0)])
        return rescale(t, torch.from_numpy(rows).cuda())
    plain_lr = [degrade(hr[None].cuda(), Degradation.fixed(0, 0, 0, 0, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    deg_lr = [degrade(hr[None].cuda(), Degradation.fixed(*params, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    want_alone = [trip(t) for t in plain_lr]
    want_all = [jpeg(filter2d(trip(t), flt, bank), q40, "420") for t in deg_lr]
    ref = refs.rescale_reference(plain_lr[0].cpu().numpy(), rescale_rows([(22, 19)], ("bicubic", "bicubic"), 0, 0, 0, [(0, 0)]))
    assert plain_lr[0].shape[2:] == (32, 28) and np.abs(255 * (want_alone[0].cpu().double().numpy() - ref)).max() <= 1.0 + 1e-3
    assert not torch.equal(want_alone[0], plain_lr[0])
    fed = []
    hook = G.register_forward_pre_hook(lambda mod, args: fed.append(args[0].clone()))
    metrics_file = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, "val", "_metrics.txt")
    results = {}
    for on_device in (False, True):
        loader = DeviceTestSet.from_dataset(ds, "cuda") if on_device else DataLoader(ds, batch_size=1, shuffle=False)
        for tile in (0, 24):
            plain = _validate(G, loader, cfg, on_device=on_device, tile=tile)
            capsys.readouterr()
            fed.clear()
            alone = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade_resize=s)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = resize(bicubic(GT)): resize round trip at scale 0.7 (bicubic) | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:                                # (tiled: the generator sees windows of the same input)
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_alone))
            fed.clear()
            every = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade=params, degrade_jpeg=40,
                              degrade_sinc=omega, degrade_resize=s)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = ("LR = degrade(GT): sigma 0.6 / 3.5, theta 30 deg, noise 10, resize round trip at scale 0.7 (bicubic), sinc cutoff 1.5, "
                    "JPEG quality 40 (420) | ")
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_all))
            _validate(G, loader, cfg, on_device=on_device, tile=tile, degrade_jpeg=40, degrade_resize=s)
            assert capsys.readouterr().out.startswith("[Test] | LR = jpeg(resize(bicubic(GT))): resize round trip at scale 0.7 (bicubic), "
                                                      "JPEG quality 40 (420) | PSNR: ")
            cfg.DATA.VALIDATE_DEGRADE_RESIZE = s
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == alone
            cfg.DATA.VALIDATE_DEGRADE_RESIZE = None
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == plain
            assert len({plain, alone, every}) == 3 and all(math.isfinite(v) for v in alone + every)
            results[on_device, tile] = (alone, every)
    hook.remove()
    for tile in (0, 24):                                 # the host and the device metric paths agree
        for a, b in zip(results[False, tile], results[True, tile]):
            assert all(abs(u - v) <= 1e-6 * abs(u) for u, v in zip(a, b))
    for on_device in (False, True):                     # the tiled forward is the whole-image forward
        for a, b in zip(results[on_device, 0], results[on_device, 24]):
            assert all(abs(u - v) <= 1e-3 * abs(u) for u, v in zip(a, b))
