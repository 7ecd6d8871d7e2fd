"""GPU: the second-order degradation stage (csrc/filter.hip: sst_filter2d; srganst.device_data: filter2d, second_order, SecondOrder,
DeviceCropLoader(second=...); validate's degrade_sinc) against the fp64 restatement of tests/filter_refs.py and its derived bound."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import filter_refs as refs
from test_degrade_gpu import _TwoPairs, _arena

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 3), (7, 9, 7), (11, 11, 21), (24, 24, 21), (33, 40, 7), (33, 40, 21), (65, 31, 13)]
IDX = {n: i for i, n in enumerate(["aniso", "generalized", "plateau", "sinc_pi3", "sinc_pi", "support", "one_hot"])}


def _rows(spec):
    """[(kernel name or None, noise255, shot, gray, key)] -> int32 [n, 8]."""
    from srganst.device_data import filter_rows
    return torch.from_numpy(filter_rows([-1 if s[0] is None else IDX[s[0]] for s in spec], [s[1] for s in spec], [s[2] for s in spec],
                                        [s[3] for s in spec], [(s[4], s[4] * 7919 + 1) for s in spec]))


# the row sets of the restatement cases: B = 1 with all stages together; B = 3 mixing pass-through, blur only, colour, gray and shot
# noise; every kernel of the bank appears
ROW_SETS = [
    [("sinc_pi", 10.0, 0.01, 1, 11)],
    [(None, 0.0, 0.0, 0, 1), ("aniso", 0.0, 0.0, 0, 2), (None, 20.0, 0.0, 0, 3)],
    [("generalized", 15.0, 0.0, 1, 4), ("plateau", 0.0, 0.02, 0, 5), ("sinc_pi3", 5.0, 0.025, 1, 6)],
    [("support", 0.0, 0.0, 0, 7), ("one_hot", 0.0, 0.0, 0, 8), ("sinc_pi", 25.0, 0.0, 0, 9)],
]


@functools.lru_cache(maxsize=None)
def _bank(K):
    bank, names = refs.case_bank(K)
    assert names == list(IDX)
    return bank


@functools.lru_cache(maxsize=None)
def _input(B, h, w):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + B)
    return torch.rand(B, 3, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(h, w, K, which):
    """The unquantised fp64 restatement of one row set on the shared input: computed once, read by every test that needs it."""
    rows = _rows(ROW_SETS[which])
    ref = refs.filter_reference(_input(len(rows), h, w).numpy(), rows.numpy(), _bank(K), quantise=False)
    ref.setflags(write=False)
    return ref


def _run(x, rows, bank, **kw):
    from srganst.device_data import filter2d
    return filter2d(x.cuda(), rows.cuda(), None if bank is None else torch.from_numpy(bank).cuda(), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("h, w, K", SHAPES)
def test_kernel_against_the_restatement(h, w, K):
    """Unquantised output within the derived bound of the restatement; quantised output = round(255 clamp(v)) / 255 taken in fp32 from
    the unquantised launch (so the quantiser is held without an ambiguity allowance); the one-hot kernel's output is the reflect-shifted
    input exactly; a pass-through sample keeps its bits."""
    bank = _bank(K)
    worst = 0.0
    for which, spec in enumerate(ROW_SETS):
        rows, x = _rows(spec), _input(len(spec), h, w)
        raw = _run(x, rows, bank, quantise=False).cpu()
        ref = _reference(h, w, K, which)
        bound = refs.bound(K, bank, rows.numpy())
        err = float(np.abs(raw.double().numpy() - ref).max())
        worst = max(worst, err / bound)
        print(f"filter2d {h}x{w} K = {K} rows {which}: max |kernel - fp64| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (which, err, bound)
        q = _run(x, rows, bank).cpu()
        for b, s in enumerate(spec):
            if s[0] is None and s[1] == 0 and s[2] == 0:
                assert torch.equal(_bits(raw[b]), _bits(x[b])) and torch.equal(_bits(q[b]), _bits(x[b]))
            else:
                assert torch.equal(q[b], torch.round(255 * raw[b].clamp(0, 1)) / 255), (which, b)
                assert float(q[b].min()) >= 0 and float(q[b].max()) <= 1
            if s[0] == "one_hot":
                assert torch.equal(raw[b], torch.from_numpy(refs.shifted(x[b].numpy(), K, *refs.one_hot_at(K))))
    print(f"filter2d {h}x{w} K = {K}: worst error / bound = {worst:.3f}")


def test_pass_through_keeps_every_bit():
    h, w, K = 33, 40, 7
    x = (_input(3, h, w) - 0.5) * 4
    x[0, 1, 3, 5], x[0, 2, 32, 39], x[2, 0, 0, 0], x[2, 1, 16, 20] = float("nan"), float("inf"), float("-inf"), float("nan")
    _bits(x)[0, 0, 0, 1] = 0x7FC01234                       # a NaN with a payload
    rows = _rows([(None, 0, 0, 0, 1), ("aniso", 0, 0, 0, 2), (None, 0, 0, 1, 3)])          # (the gray flag alone is no noise)
    for quantise in (True, False):
        out = _run(x, rows, _bank(K), quantise=quantise).cpu()
        assert torch.equal(_bits(out[0]), _bits(x[0])) and torch.equal(_bits(out[2]), _bits(x[2]))
        assert bool(torch.isfinite(out[1]).all()) and (not quantise or (float(out[1].min()) >= 0 and float(out[1].max()) <= 1))
    # without a bank: M = 0, a null pointer
    out = _run(x, _rows([(None, 0, 0, 0, 1)] * 3), None).cpu()
    assert torch.equal(_bits(out), _bits(x))


def test_noise_without_a_bank_and_on_a_tiny_image():
    """M = 0 is legal (noise only), also where the window would not fit the image."""
    from srganst.device_data import filter2d, filter_rows
    x = _input(2, 2, 2)
    rows = torch.from_numpy(filter_rows([-1, -1], [12.0, 0.0], [0.0, 0.02], [0, 1], [(3, 4), (5, 6)]))
    raw = _run(x, rows, None, quantise=False).cpu()
    ref = refs.filter_reference(x.numpy(), rows.numpy(), None, quantise=False)
    assert np.abs(raw.double().numpy() - ref).max() <= refs.bound(3, None, rows.numpy())
    empty = torch.zeros(0, 21, 21, device="cuda")
    assert torch.equal(filter2d(x.cuda(), rows.cuda(), empty, quantise=False).cpu(), raw)


def test_gray_noise_is_one_draw_for_the_three_channels():
    h, w, K = 33, 40, 21
    x = _input(1, h, w)[:, :1].expand(2, 3, h, w).contiguous()
    spec = [("plateau", 20.0, 0.01, 1, 5), ("plateau", 20.0, 0.01, 0, 5)]
    for quantise in (False, True):
        out = _run(x, _rows(spec), _bank(K), quantise=quantise)
        assert torch.equal(out[0, 0], out[0, 1]) and torch.equal(out[0, 0], out[0, 2])
        assert not torch.equal(out[1, 0], out[1, 1]) and not torch.equal(out[1, 1], out[1, 2])
        assert torch.equal(out[0, 0], out[1, 0])                                  # e = y * w + x: channel 0's draws


def test_a_sample_sees_its_key_but_neither_its_position_the_batch_nor_the_tiles(monkeypatch):
    from srganst.device_data import filter2d
    h, w, K = 33, 40, 21
    spec = [("sinc_pi3", 8.0, 0.0, 0, 1), (None, 0.0, 0.0, 0, 2), ("aniso", 0.0, 0.02, 1, 3), ("one_hot", 12.0, 0.0, 0, 4),
            (None, 9.0, 0.01, 0, 5)]
    x, rows, bank = _input(5, h, w).cuda(), _rows(spec).cuda(), torch.from_numpy(_bank(K)).cuda()
    a = filter2d(x, rows, bank)
    assert torch.equal(filter2d(x, rows, bank), a)                                  # same inputs, same bits
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    assert torch.equal(filter2d(x[perm].contiguous(), rows[perm].contiguous(), bank), a[perm])
    assert torch.equal(filter2d(x[2:3].contiguous(), rows[2:3].contiguous(), bank)[0], a[2])
    rekeyed = rows.clone()
    rekeyed[:, 4] += 1
    b = filter2d(x, rekeyed, bank)
    assert torch.equal(b[1], a[1]) and all(not torch.equal(b[i], a[i]) for i in (0, 2, 3, 4))
    # the tile geometry: 32-row tiles (one workgroup would hold the training shape), the launcher's choice, and bands of 8, 5 and 1
    raw = filter2d(x, rows, bank, quantise=False)
    for tile_rows in ("32", "8", "5", "1"):
        monkeypatch.setenv("SST_FILTER_ROWS", tile_rows)
        assert torch.equal(filter2d(x, rows, bank), a) and torch.equal(filter2d(x, rows, bank, quantise=False), raw), tile_rows
    monkeypatch.delenv("SST_FILTER_ROWS")
    # the forms: a new tensor (the input untouched), out=; out is x raises; a non-contiguous input is read as it is indexed
    keep = x.clone()
    o = torch.full_like(x, 7.0)
    assert filter2d(x, rows, bank, out=o) is o and torch.equal(o, a) and torch.equal(x, keep)
    with pytest.raises(ValueError, match="out must not be x"):
        filter2d(x, rows, bank, out=x)
    wide = torch.zeros(5, 3, h, 50, device="cuda")
    wide[..., :w] = x
    assert torch.equal(filter2d(wide[..., :w], rows, bank), a)
    with pytest.raises(ValueError, match="out must be contiguous fp32"):
        filter2d(x, rows, bank, out=wide[..., :w])
    with pytest.raises(ValueError, match="bank must be contiguous fp32"):
        filter2d(x, rows, bank.double())
    with pytest.raises(ValueError, match="deg must be contiguous int32"):
        filter2d(x, rows[:4], bank)


def test_nan_conventions_touch_that_sample_only():
    from srganst.device_data import filter2d
    h, w, K = 33, 40, 7
    spec = [("aniso", 5.0, 0.0, 0, 1), ("plateau", 0.0, 0.01, 1, 2), (None, 0.0, 0.0, 0, 3)]
    x, bank = _input(3, h, w).cuda(), torch.from_numpy(_bank(K)).cuda()
    good = _rows(spec)
    clean = filter2d(x, good.cuda(), bank)
    f32 = lambda v: int(np.float32(v).view(np.int32))
    for word, value in ((0, -2), (0, len(IDX)), (0, 1 << 30), (0, -(1 << 31)), (3, 2), (3, -1), (3, 256), (1, f32(-1e-3)), (1, f32("nan")),
                        (2, f32(-1.0)), (2, f32("nan")), (1, f32("-inf"))):
        for victim in (0, 1, 2):
            rows = good.clone()
            rows[victim, word] = value
            out = filter2d(x, rows.cuda(), bank)
            assert bool(torch.isnan(out[victim]).all()), (word, value, victim)
            for other in set(range(3)) - {victim}:
                assert torch.equal(out[other], clean[other]), (word, value, victim, other)
    # with no bank every index but -1 is outside [-1, 0)
    rows = good.clone()
    rows[:, 0] = torch.tensor([0, -1, -1])
    out = filter2d(x, rows.cuda(), None)
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isfinite(out[1]).all()) and torch.equal(out[2], x[2])
    # a NaN pixel spreads over its window and no further
    dirty = x.clone()
    dirty[0, 1, 16, 20] = float("nan")
    out = filter2d(dirty, good.cuda(), bank)
    mask = torch.zeros(3, h, w, dtype=torch.bool, device="cuda")
    mask[1, 13:20, 17:24] = True
    assert bool(torch.isnan(out[0][mask]).all()) and torch.equal(out[0][~mask], clean[0][~mask]) and torch.equal(out[1:], clean[1:])


def test_captured_launch_replayed_on_fresh_data_and_rows():
    from srganst.device_data import filter2d
    h, w, K = 33, 40, 21
    bank = torch.from_numpy(_bank(K)).cuda()
    spec = [("sinc_pi", 10.0, 0.0, 0, 1), (None, 0.0, 0.0, 0, 2), ("support", 0.0, 0.02, 1, 3)]
    x, rows = _input(3, h, w).cuda(), _rows(spec).cuda()
    want = filter2d(x, rows, bank)
    buf, out = x.clone(), torch.zeros_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, one kernel node
        filter2d(buf, rows, bank, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    fresh = (_input(3, h, w).flip(0) * 0.9).contiguous().cuda()
    fresh_rows = _rows([("aniso", 0.0, 0.0, 0, 7), ("generalized", 3.0, 0.0, 1, 8), (None, 0.0, 0.0, 0, 9)]).cuda()
    buf.copy_(fresh), rows.copy_(fresh_rows)                                       # the graph reads both when it runs
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, filter2d(fresh, fresh_rows, bank))


def _second(ksize, **kw):
    from srganst.device_data import SecondOrder
    return SecondOrder(ksize=ksize, bank_size=24, sinc_bank_size=8, jpeg_quality=(20, 100), **kw)


@pytest.mark.parametrize("scale, ksize", [(2, 21), (4, 7)])                        # LR 12 x 12 under K = 21; LR 6 x 6 under K = 7
def test_loader_with_the_second_stage(scale, ksize, monkeypatch):
    """Two epochs over the small arena: lr is the public ops composed by hand (filter2d, filter2d, jpeg, filter2d) on the lr and rows of
    the loader without the second stage, gt is that loader's; the last launch writes the bound buffer; an epoch repeats.  With
    second=None: the bits of before and sst_filter2d never launched."""
    from srganst import device_data
    from srganst.device_data import Degradation, DeviceCropLoader, filter2d, jpeg
    S, B = 24, 2
    _, arena, _, _ = _arena(S, scale)
    order = list(range(len(arena)))[::-1]
    first = Degradation(blur_prob=0.8, noise_prob=0.8, jpeg_prob=0.5, jpeg_chroma="444")
    so = _second(ksize, jpeg_chroma="444", jpeg_prob=0.7)
    on = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first, second=so)
    off = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first)
    gt_buf, lr_buf = torch.zeros(B, 3, S, S, device="cuda"), torch.zeros(B, 3, S // scale, S // scale, device="cuda")
    seen, stages = [], np.zeros(4, np.int64)
    for epoch in range(2):
        assert np.array_equal(on.deg_draws(epoch), off.deg_draws(epoch)) and np.array_equal(on.draws(epoch), off.draws(epoch))
        rows, bank = on.second_draws(epoch)
        bank_d = torch.from_numpy(bank).cuda()
        if epoch == 1:
            on.bind(gt_buf, lr_buf)
        n = 0
        for (gt1, lr1), (gt0, lr0) in zip(on, off):
            sel = order[n * B:(n + 1) * B]
            r = torch.from_numpy(np.ascontiguousarray(rows[:, sel])).cuda()
            stages += [(r[0, :, 0] >= 0).sum().item(), (r[1, :, 0] >= 0).sum().item(), (r[2, :, 6] > 0).sum().item(),
                       (r[3, :, 0] >= 0).sum().item()]
            want = filter2d(filter2d(lr0, r[0], bank_d), r[1], bank_d)
            want = filter2d(jpeg(want, r[2], "444"), r[3], bank_d)
            assert torch.equal(gt1, gt0) and torch.equal(lr1, want), (epoch, n)
            assert epoch == 0 or (lr1 is lr_buf and gt1 is gt_buf)
            assert torch.equal(lr1, device_data.second_order(lr0, r, bank_d, "444"))
            seen.append(lr1.clone())
            n += 1
        assert n == len(on) >= 3
    assert (stages > 0).all(), stages                                              # every stage ran on some sample
    on.bind(None, None)
    on.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(seen, on))
    # without the second stage the loader issues exactly the launches of before
    before = [lr.clone() for _, lr in DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first)]

    def boom(*a, **k):
        raise AssertionError("sst_filter2d launched by a loader without a second stage")
    monkeypatch.setattr(device_data, "filter2d", boom)
    off.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(before, off))
    with pytest.raises(AssertionError, match="without a second stage"):
        on.set_epoch(0)
        list(on)


def test_loader_with_fixed_parameters_follows_the_restatement():
    """SecondOrder.fixed through the loader against the fp64 restatement, stage by stage on the kernel's own intermediate values."""
    from srganst import kernels
    from srganst.device_data import Degradation, DeviceCropLoader, SecondOrder, filter2d
    _, arena, _, _ = _arena(24, 2)
    order = list(range(len(arena)))
    table = kernels.plateau(21, 1.2, 0.7, 0.4, beta=1.3, support=9)
    so = SecondOrder.fixed(kernel=table, noise=6.0, shot=0.004, gray=True, key=77, sinc_omega=2.2, sinc_first=False)
    first = Degradation.fixed(1.0, 2.0, 30.0, 3.0, key=5)
    on = DeviceCropLoader(arena, 4, order, degradation=first, second=so)
    off = DeviceCropLoader(arena, 4, order, degradation=first)
    rows, bank = on.second_draws(0)
    (_, lr1), (_, lr0) = next(iter(on)), next(iter(off))
    r = rows[:, :4]
    a_raw = filter2d(lr0, torch.from_numpy(np.ascontiguousarray(r[0])).cuda(), torch.from_numpy(bank).cuda(), quantise=False)
    ref = refs.filter_reference(lr0.cpu().numpy(), r[0], bank, quantise=False)
    assert np.abs(a_raw.cpu().double().numpy() - ref).max() <= refs.bound(21, bank, r[0])
    a = (torch.round(255 * a_raw.cpu().clamp(0, 1)) / 255).cuda()
    c_raw = filter2d(a, torch.from_numpy(np.ascontiguousarray(r[3])).cuda(), torch.from_numpy(bank).cuda(), quantise=False)
    ref = refs.filter_reference(a.cpu().numpy(), r[3], bank, quantise=False)
    assert np.abs(c_raw.cpu().double().numpy() - ref).max() <= refs.bound(21, bank, r[3])
    assert torch.equal(lr1.cpu(), torch.round(255 * c_raw.cpu().clamp(0, 1)) / 255)


def test_warmup_trains_on_second_order_batches(tmp_path, monkeypatch, capsys):
    from srganst.config import Config
    from srganst.loss import MSELoss
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    _, arena, _, _ = _arena(24, 4)
    cfg = Config()
    cfg.EXP.NAME, cfg.EXP.N_EPOCHS, cfg.EXP.SAVE_STATE = "second", 1, False
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    cfg.DATA.BATCH_SIZE, cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 2, 24, 8
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.LOG_TRAIN_PERIOD = 1
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = cfg.DATA.DEGRADE = cfg.DATA.DEGRADE_SECOND = True
    cfg.DATA.DEGRADE2_KSIZE, cfg.DATA.DEGRADE2_BANK_SIZE, cfg.DATA.DEGRADE2_SINC_BANK_SIZE = 11, 16, 8        # LR 6 x 6: p = 5
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss()}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0}
    warmup(cfg, train_dataset=arena, test_dataset=_Pairs(), max_steps_per_epoch=3)
    out = capsys.readouterr().out
    assert out.count("DATA.DEGRADE: lr = quantise") == 1
    assert out.count("DATA.DEGRADE_SECOND: then lr = sinc(jpeg(sinc(quantise(clamp(lr * k2 + n2)))))") == 1 and "ksize=11, bank_size=16+8" in out
    losses = [float(v) for m in re.findall(r"\[G losses: \{([^}]*)\}", out) for v in re.findall(r": ([-+0-9.einfa]+)", m)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    assert os.path.exists("results/second/g_last.pth")


def test_validation_with_degrade_sinc(tmp_path, capsys):
    """Both validation paths, whole and tiled: the input is the sinc filter of degrade(gt) (or of the plain bicubic LR made from gt), before
    the JPEG stage when there is one; the head line names the cutoff; off: the numbers of before."""
    from torch.utils.data import DataLoader
    from srganst import kernels
    from srganst.config import Config
    from srganst.device_data import Degradation, DeviceTestSet, degrade, filter2d, filter_rows, jpeg
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    cfg.EXP.NAME = "val"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    ds = _TwoPairs()
    params, omega = (0.6, 3.5, 30.0, 10.0), 1.5
    bank = torch.from_numpy(kernels.bank([kernels.sinc(21, omega)])).cuda()
    flt = torch.from_numpy(filter_rows([0], 0, 0, 0, [(0, 0)])).cuda()
    q40 = torch.zeros(1, 8, dtype=torch.int32, device="cuda")
    q40[0, 6] = 40
    plain_lr = [degrade(hr[None].cuda(), Degradation.fixed(0, 0, 0, 0, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    deg_lr = [degrade(hr[None].cuda(), Degradation.fixed(*params, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    want_alone = [filter2d(t, flt, bank) for t in plain_lr]
    want_all = [jpeg(filter2d(t, flt, bank), q40, "420") for t in deg_lr]
    ref = refs.filter_reference(plain_lr[0].cpu().numpy(), flt.cpu().numpy(), bank.cpu().numpy(), quantise=False)
    assert np.abs(255 * want_alone[0].cpu().double().numpy() - np.rint(255 * np.clip(ref, 0, 1))).max() <= 1.0 + 1e-3
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
            alone = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade_sinc=omega)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = sinc(bicubic(GT)): sinc cutoff 1.5 | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:                                # (tiled: the generator sees windows of the same input)
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_alone))
            fed.clear()
            every = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade=params, degrade_jpeg=40,
                              degrade_sinc=omega)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = degrade(GT): sigma 0.6 / 3.5, theta 30 deg, noise 10, sinc cutoff 1.5, JPEG quality 40 (420) | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_all))
            _validate(G, loader, cfg, on_device=on_device, tile=tile, degrade_jpeg=40, degrade_sinc=omega)
            assert capsys.readouterr().out.startswith("[Test] | LR = jpeg(sinc(bicubic(GT))): sinc cutoff 1.5, JPEG quality 40 (420) | PSNR: ")
            cfg.DATA.VALIDATE_DEGRADE_SINC = omega
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == alone
            cfg.DATA.VALIDATE_DEGRADE_SINC = None
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
