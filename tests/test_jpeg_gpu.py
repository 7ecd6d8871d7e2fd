"""GPU: the JPEG stage of the degradation (csrc/jpeg.hip: sst_jpeg; srganst.device_data: jpeg, degrade(jpeg_chroma=...),
DeviceImageArena.crops(jpeg_chroma=...), DeviceCropLoader with a Degradation that draws qualities; validate's degrade_jpeg) against
the integer restatement of tests/jpeg_refs.py.  The codec is int32 arithmetic at every step, so every comparison is bit for bit."""
import math
import os
import re

import numpy as np
import pytest
import torch

import jpeg_refs as refs
from test_degrade_gpu import _TwoPairs, _arena, _mixed_rows

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 13), (24, 24), (33, 40)]      # the last: one pixel past a 32-px tile, a partial MCU
MODES = ["444", "420"]


def _rows(qualities):
    """deg rows that hold only a JPEG quality each."""
    deg = torch.zeros(len(qualities), 8, dtype=torch.int32)
    deg[:, 6] = torch.tensor(qualities, dtype=torch.int32)
    return deg


def _batch(B, h, w, seed=0):
    """fp32 [B, 3, h, w] on the 1/255 grid: the fixtures' smooth image with its edge first, then uniform noise."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    x = torch.randint(0, 256, (B, 3, h, w), generator=g).float() / 255
    x[0] = torch.from_numpy(refs.fixture_image(h, w, seed)).permute(2, 0, 1).float() / 255
    return x


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    want = torch.from_numpy(want)
    got = got.cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def _run(x, deg, mode):
    from srganst.device_data import jpeg
    return jpeg(x.cuda(), deg.cuda(), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h, w", SIZES)
def test_kernel_against_the_restatement(h, w, mode):
    """B = 1, and B = 3 with mixed rows: Q = 0 keeps the bits; 1, 50, 75 and 100 equal the restatement."""
    for qualities in ([75], [0, 1, 50], [100, 50, 0]):
        x, deg = _batch(len(qualities), h, w), _rows(qualities)
        out = _run(x, deg, mode)
        assert torch.equal(out.cpu(), torch.from_numpy(refs.jpeg_reference(x.numpy(), deg.numpy(), mode, tile=refs.TILE))), qualities
        for b, Q in enumerate(qualities):
            assert (Q != 0) or torch.equal(out[b].cpu(), x[b])
    assert float(out.min()) >= 0 and float(out.max()) <= 1


@pytest.mark.parametrize("mode", MODES)
def test_checkerboards_and_inputs_off_the_grid(mode):
    deg = _rows([1, 50, 100])
    for h, w, period in ((33, 40, 1), (24, 24, 2), (16, 16, 1), (17, 13, 4)):
        x = torch.from_numpy(np.stack([refs.checkerboard(h, w, period)] * 3))
        assert torch.equal(_run(x, deg, mode).cpu(), torch.from_numpy(refs.jpeg_reference(x.numpy(), deg.numpy(), mode)))
    # off the grid and outside [0, 1]: the codec sees rint(255 clamp01(v)); Q = 0 keeps even these bits
    x = (_batch(3, 33, 40, seed=2) - 0.5) * 3 + 0.001
    deg = _rows([60, 0, 35])
    out = _run(x, deg, mode)
    assert torch.equal(out.cpu(), torch.from_numpy(refs.jpeg_reference(x.numpy(), deg.numpy(), mode))) and torch.equal(out[1].cpu(), x[1])
    snapped = torch.round(255 * x.clamp(0, 1)) / 255
    assert torch.equal(out[[0, 2]], _run(snapped, deg, mode)[[0, 2]])


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_elements_and_qualities_out_of_range(mode):
    M = 8 if mode == "444" else 16
    x = _batch(3, 33, 40, seed=3)
    deg = _rows([50, 50, 50])
    clean = _run(x, deg, mode)
    dirty = x.clone()
    spots = [(0, 1, 9, 20, float("nan")), (1, 0, 32, 39, float("inf")), (2, 2, 0, 0, float("-inf")), (2, 1, 31, 31, float("nan"))]
    for b, c, y, xx, v in spots:
        dirty[b, c, y, xx] = v
    out = _run(dirty, deg, mode)
    assert _same(out, refs.jpeg_reference(dirty.numpy(), deg.numpy(), mode))
    mask = torch.zeros_like(x, dtype=torch.bool)
    for b, c, y, xx, v in spots:
        mask[b, :, y // M * M:y // M * M + M, xx // M * M:xx // M * M + M] = True
    assert bool(torch.isnan(out.cpu()[mask]).all()) and torch.equal(out.cpu()[~mask], clean.cpu()[~mask])
    # a quality outside 0..100: that sample is NaN, the others are untouched by it
    for bad in (-1, 101, 1 << 30, -(1 << 31)):
        out = _run(x, _rows([50, bad, 0]), mode)
        assert bool(torch.isnan(out[1]).all()) and torch.equal(out[0], clean[0]) and torch.equal(out[2].cpu(), x[2])


@pytest.mark.parametrize("mode", MODES)
def test_a_sample_sees_neither_its_position_nor_the_batch(mode):
    from srganst.device_data import jpeg
    x, deg = _batch(5, 33, 40, seed=4).cuda(), _rows([30, 0, 95, 1, 70]).cuda()
    a = jpeg(x, deg, mode)
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    assert torch.equal(jpeg(x[perm].contiguous(), deg[perm].contiguous(), mode), a[perm])
    assert torch.equal(jpeg(x[2:3].contiguous(), deg[2:3].contiguous(), mode)[0], a[2])
    assert torch.equal(jpeg(x, deg, mode), a)                                     # same inputs, same bits
    # the forms: a new tensor (the input untouched), out=, and in place
    keep = x.clone()
    o = torch.full_like(x, 7.0)
    assert jpeg(x, deg, mode, out=o) is o and torch.equal(o, a) and torch.equal(x, keep)
    assert jpeg(x, deg, mode, out=x) is x and torch.equal(x, a)
    # a non-contiguous input is read as it is indexed
    wide = torch.zeros(5, 3, 33, 50, device="cuda")
    wide[..., :40] = keep
    assert torch.equal(jpeg(wide[..., :40], deg, mode), a)
    with pytest.raises(ValueError, match="out must be contiguous fp32"):
        jpeg(keep, deg, mode, out=wide[..., :40])


@pytest.mark.parametrize("mode", MODES)
def test_captured_launch_replayed_on_fresh_data(mode):
    from srganst.device_data import jpeg
    x, deg = _batch(3, 33, 40, seed=5).cuda(), _rows([40, 0, 90]).cuda()
    want = jpeg(x, deg, mode)
    buf = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, one kernel node, in place
        jpeg(buf, deg, mode, out=buf)
    for _ in range(2):
        buf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, want)
    fresh, fresh_deg = _batch(3, 33, 40, seed=6), _rows([0, 15, 100])
    buf.copy_(fresh.cuda()), deg.copy_(fresh_deg.cuda())                          # the graph reads both when it runs
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.from_numpy(refs.jpeg_reference(fresh.numpy(), fresh_deg.numpy(), mode)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S, scale, K", [(24, 4, 21), (32, 2, 9), (24, 2, 7)])       # LR 6 x 6, 16 x 16, 12 x 12
def test_crops_and_degrade_with_jpeg(S, scale, K, mode):
    """crops(desc, deg, jpeg_chroma)'s lr equals degrade(its gt, deg, jpeg_chroma) bit for bit: all eight transforms, blur, noise and
    JPEG on; and both equal the restatement applied to the lr made without the JPEG stage."""
    from srganst.device_data import degrade
    _, arena, batch, desc = _arena(S, scale)
    deg = _mixed_rows(len(batch), K, noise=True)
    deg[:, 6] = torch.tensor([30, 95, 0, 50, 1, 100, 75, 10][:len(batch)], dtype=torch.int32)
    deg = deg.cuda()
    gt0, lr0 = arena.crops(desc, deg=deg, ksize=K)
    gt, lr = arena.crops(desc, deg=deg, ksize=K, jpeg_chroma=mode)
    assert torch.equal(gt, gt0) and torch.equal(lr, degrade(gt, deg, scale, K, jpeg_chroma=mode))
    assert torch.equal(lr.cpu(), torch.from_numpy(refs.jpeg_reference(lr0.cpu().numpy(), deg.cpu().numpy(), mode)))
    assert torch.equal(lr[2], lr0[2]) and not torch.equal(lr[0], lr0[0])
    assert torch.equal(degrade(gt, deg, scale, K), lr0)                           # without the option: the launch and bits of before
    with pytest.raises(ValueError, match="jpeg_chroma needs deg"):
        arena.crops(desc, jpeg_chroma=mode)
    with pytest.raises(ValueError, match="jpeg_chroma needs deg"):
        arena.crops(desc, deg=deg, ksize=K, quantise=False, jpeg_chroma=mode)


def test_loader_with_jpeg_qualities(monkeypatch):
    """Two epochs over the small arena: lr is the restatement applied to the lr of the loader whose Degradation draws no quality (the
    same first six words); with jpeg_prob = 0 the loader's output is degrade() without the JPEG stage and sst_jpeg is never launched."""
    from srganst import device_data
    from srganst.device_data import Degradation, DeviceCropLoader, degrade
    S, scale, B = 24, 4, 2
    _, arena, _, _ = _arena(S, scale)
    order = list(range(len(arena)))[::-1]
    on = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=Degradation(blur_prob=0.8, noise_prob=0.8, jpeg_prob=0.7,
                                                                                        jpeg_quality=(5, 100), jpeg_chroma="444"))
    off = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=Degradation(blur_prob=0.8, noise_prob=0.8))
    seen, n_jpeg = [], 0
    for epoch in range(2):
        rows, rows_off = on.deg_draws(epoch), off.deg_draws(epoch)
        assert np.array_equal(rows[:, :6], rows_off[:, :6]) and (rows_off[:, 6:] == 0).all()
        n = 0
        for (gt1, lr1), (gt0, lr0) in zip(on, off):
            deg = rows[order[n * B:(n + 1) * B]]
            n_jpeg += int((deg[:, 6] > 0).sum())
            assert torch.equal(gt1, gt0)
            assert torch.equal(lr1.cpu(), torch.from_numpy(refs.jpeg_reference(lr0.cpu().numpy(), deg, "444")))
            # jpeg_prob = 0: the parent's behaviour, degrade() of its gt without the JPEG stage
            assert torch.equal(lr0, degrade(gt0, torch.from_numpy(rows_off[order[n * B:(n + 1) * B]]).cuda(), scale, 21))
            seen.append(lr1.clone())
            n += 1
        assert n == len(on) >= 3
    assert 0 < n_jpeg < 2 * len(on) * B
    on.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(seen, on))
    # without qualities the loader issues exactly the launch of before
    def boom(*a, **k):
        raise AssertionError("sst_jpeg launched by a loader whose Degradation draws no quality")
    monkeypatch.setattr(device_data, "jpeg", boom)
    off.set_epoch(0)
    assert len(list(off)) == len(off)
    with pytest.raises(AssertionError, match="draws no quality"):
        on.set_epoch(0)
        list(on)


def test_warmup_trains_on_jpeg_degraded_batches(tmp_path, monkeypatch, capsys):
    from srganst.config import Config
    from srganst.loss import MSELoss
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    _, arena, _, _ = _arena(24, 4)
    cfg = Config()
    cfg.EXP.NAME, cfg.EXP.N_EPOCHS, cfg.EXP.SAVE_STATE = "jpeg", 1, False
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    cfg.DATA.BATCH_SIZE, cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 2, 24, 8
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.LOG_TRAIN_PERIOD = 1
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = cfg.DATA.DEGRADE = True
    cfg.DATA.DEGRADE_JPEG_PROB, cfg.DATA.DEGRADE_JPEG_QUALITY = 1.0, (20, 60)
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss()}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0}
    warmup(cfg, train_dataset=arena, test_dataset=_Pairs(), max_steps_per_epoch=3)
    out = capsys.readouterr().out
    assert out.count("DATA.DEGRADE: lr = quantise") == 1 and "jpeg_quality=(20, 60), jpeg_prob=1, jpeg_chroma='420'" in out
    assert out.count("then lr = jpeg(lr) in a second launch (sst_jpeg, integer codec, chroma 420)") == 1
    losses = [float(v) for m in re.findall(r"\[G losses: \{([^}]*)\}", out) for v in re.findall(r": ([-+0-9.einfa]+)", m)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    assert os.path.exists("results/jpeg/g_last.pth")


def test_validation_with_degrade_jpeg(tmp_path, capsys):
    """Both validation paths, whole and tiled: alone the input is the JPEG stage of the plain bicubic LR made from gt, with
    VALIDATE_DEGRADE that of degrade(gt); the head line names the quality."""
    from torch.utils.data import DataLoader
    from srganst.config import Config
    from srganst.device_data import Degradation, DeviceTestSet, degrade
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    cfg.EXP.NAME = "val"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    ds = _TwoPairs()
    params = (0.6, 3.5, 30.0, 10.0)
    q40 = _rows([40])
    plain_lr = [degrade(hr[None].cuda(), Degradation.fixed(0, 0, 0, 0, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    deg_lr = [degrade(hr[None].cuda(), Degradation.fixed(*params, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    want_alone = [torch.from_numpy(refs.jpeg_reference(t.cpu().numpy(), q40.numpy(), "420")) for t in plain_lr]
    want_both = [torch.from_numpy(refs.jpeg_reference(t.cpu().numpy(), q40.numpy(), "420")) for t in deg_lr]
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
            alone = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade_jpeg=40)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = jpeg(bicubic(GT)): JPEG quality 40 (420) | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:                                # (tiled: the generator sees windows of the same input)
                assert len(fed) == 2 and all(torch.equal(a.cpu(), b) for a, b in zip(fed, want_alone))
            fed.clear()
            both = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade=params, degrade_jpeg=40)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = degrade(GT): sigma 0.6 / 3.5, theta 30 deg, noise 10, JPEG quality 40 (420) | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:
                assert len(fed) == 2 and all(torch.equal(a.cpu(), b) for a, b in zip(fed, want_both))
            cfg.DATA.VALIDATE_DEGRADE_JPEG = 40
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == alone
            cfg.DATA.VALIDATE_DEGRADE_JPEG = None
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == plain
            assert len({plain, alone, both}) == 3 and all(math.isfinite(v) for v in alone + both)
            results[on_device, tile] = (alone, both)
    hook.remove()
    for tile in (0, 24):                                 # the host and the device metric paths agree
        for a, b in zip(results[False, tile], results[True, tile]):
            assert all(abs(u - v) <= 1e-6 * abs(u) for u, v in zip(a, b))
    for on_device in (False, True):                     # the tiled forward is the whole-image forward
        for a, b in zip(results[on_device, 0], results[on_device, 24]):
            assert all(abs(u - v) <= 1e-3 * abs(u) for u, v in zip(a, b))
