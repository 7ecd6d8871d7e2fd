"""GPU: validation on the device - sst_image_metrics (csrc/metrics.hip) against the host path it restates, never against itself.

The yardstick of every comparison is validate.image_metrics / utils.tensor2img on the same tensors (their PSNR / Y / tensor2img
parts are pinned to the reference by tests/golden/metrics.npz).  Bounds: the uint8 images are equal, no tolerance; PSNR and SSIM
within 1e-6 of the host values, the bound the project pins these metrics with (tests/test_host_logic.py).  With both fp32 roundings
of Y reproduced the expected difference is fp64 summation order only; every test prints what it measured.

Measured on MI355X (PyTorch 2.10, ROCm 7.0), maximum over all cases of this file: |dPSNR| = 0 (every PSNR equal to the last bit),
|dSSIM| = 1.1e-14 (the 11 x 11 image; 2.8e-15 on the larger ones); _validate's averages differ by 0 dB and 1.7e-17."""
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

pytestmark = pytest.mark.gpu

BOUND = 1e-6
SIZES = ((48, 64), (72, 40), (96, 96), (211, 173), (11, 11))
NOISE = (0.05, 0.2, 0.01, 0.1, 0.1)


def _smooth_hr(h, w, g, batch=1):
    """tests/test_drivers_gpu.py:_Pairs's HR: bicubic-smooth, on the 1/255 grid."""
    base = torch.rand(batch, 3, max(h // 8, 2), max(w // 8, 2), generator=g)
    hr = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)
    return torch.round(hr * 255) / 255


def _pair(h, w, noise, seed, batch=1):
    g = torch.Generator().manual_seed(seed)
    hr = _smooth_hr(h, w, g, batch)
    return hr + noise * torch.randn(hr.shape, generator=g), hr


def _host(sr, hr):
    """[(psnr, ssim, sr_u8, hr_u8)] per image by the host path."""
    from srganst.utils import tensor2img
    from srganst.validate import image_metrics
    rows = []
    for b in range(sr.shape[0]):
        p, s = image_metrics(sr[b:b + 1].clone(), hr[b:b + 1].clone())
        rows.append((p, s, tensor2img(sr[b:b + 1].clone()), tensor2img(hr[b:b + 1].clone())))
    return rows


def _device(sr, hr):
    from srganst.metrics import image_metrics_device, psnr_from_mse
    out, s8, h8 = image_metrics_device(sr.cuda(), hr.cuda(), want_u8=True)
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (sr.shape[0], 2)
    assert s8.dtype == torch.uint8 and tuple(s8.shape) == (sr.shape[0], sr.shape[2], sr.shape[3], 3)
    o = out.cpu()
    return [(psnr_from_mse(o[b, 0].item()), o[b, 1].item(), s8[b].cpu().numpy(), h8[b].cpu().numpy()) for b in range(sr.shape[0])]


def _compare(name, sr, hr):
    worst = [0.0, 0.0]
    for b, (d, h) in enumerate(zip(_device(sr, hr), _host(sr, hr))):
        dp = 0.0 if d[0] == h[0] else abs(d[0] - h[0])
        ds = abs(d[1] - h[1])
        print(f"{name}[{b}]: host PSNR {h[0]:.6f} SSIM {h[1]:.8f}   |dPSNR| {dp:.3e}  |dSSIM| {ds:.3e}")
        assert np.array_equal(d[2], h[2]), f"{name}[{b}]: sr_u8 differs from tensor2img"
        assert np.array_equal(d[3], h[3]), f"{name}[{b}]: hr_u8 differs from tensor2img"
        assert dp <= BOUND and ds <= BOUND, (name, b, d[:2], h[:2])
        worst = [max(worst[0], dp), max(worst[1], ds)]
    return worst


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_metrics_match_the_host_path(k):
    (h, w), noise = SIZES[k], NOISE[k]
    sr, hr = _pair(h, w, noise, seed=20 + k)
    rows = _host(sr, hr)
    assert 10.0 < rows[0][0] < 60.0 and 0.1 < rows[0][1] < 0.999           # far from degenerate
    _compare(f"{h}x{w} noise {noise}", sr, hr)


def test_identical_images_give_zero_mse_and_ssim_one():
    from srganst.metrics import image_metrics_device, psnr_from_mse
    _, hr = _pair(72, 40, 0.0, seed=31)
    out = image_metrics_device(hr.cuda(), hr.clone().cuda()).cpu()
    assert out[0, 0].item() == 0.0 and out[0, 1].item() == 1.0
    assert psnr_from_mse(out[0, 0].item()) == float("inf")
    p, s = _host(hr, hr)[0][:2]
    assert p == float("inf") and s == 1.0


def test_values_outside_the_unit_interval_are_clamped():
    sr, hr = _pair(96, 96, 0.3, seed=32)
    sr = sr * 1.5 - 0.25
    assert float(sr.min()) < -0.2 and float(sr.max()) > 1.2
    _compare("clamp", sr, hr)


def test_half_way_points_round_half_to_even():
    g = torch.Generator().manual_seed(33)
    hr = _smooth_hr(48, 64, g)
    k = torch.randint(0, 255, hr.shape, generator=g).float()
    sr = (k + 0.5) / 255
    exact = (sr * 255) == k + 0.5
    assert 0.2 < float(exact.float().mean())                  # many of them ARE ties in fp32; both parities of k occur
    from srganst.utils import tensor2img
    u = tensor2img(sr.clone())[..., ::-1].transpose(2, 0, 1)
    ties = exact[0].numpy()
    assert (u[ties] % 2 == 0).all()
    _compare("half-way", sr, hr)


def test_batch_of_three_matches_per_image_and_is_reproducible():
    from srganst.metrics import image_metrics_device
    sr, hr = _pair(72, 88, 0.08, seed=34, batch=3)
    _compare("batch3", sr, hr)
    a = image_metrics_device(sr.cuda(), hr.cuda())
    b = image_metrics_device(sr.cuda(), hr.cuda())
    assert torch.equal(a, b)
    for i in range(3):                                        # a batch row = that image alone, bit for bit
        assert torch.equal(image_metrics_device(sr[i:i + 1].cuda(), hr[i:i + 1].cuda())[0], a[i])
    big_sr, big_hr = _pair(211, 173, 0.1, seed=35)
    assert torch.equal(image_metrics_device(big_sr.cuda(), big_hr.cuda()), image_metrics_device(big_sr.cuda(), big_hr.cuda()))


@pytest.mark.parametrize("where", ["sr", "hr"])
def test_nan_poisons_exactly_its_image(where):
    from srganst.metrics import image_metrics_device
    sr, hr = _pair(72, 88, 0.08, seed=36, batch=3)
    clean, s8c, h8c = image_metrics_device(sr.cuda(), hr.cuda(), want_u8=True)
    bad_sr, bad_hr = sr.clone(), hr.clone()
    (bad_sr if where == "sr" else bad_hr)[1, 0, 70, 3] = float("nan")        # channel R, in the last tile row
    out, s8, h8 = image_metrics_device(bad_sr.cuda(), bad_hr.cuda(), want_u8=True)
    assert torch.isnan(out[1]).all()
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    hit, hit_c = (s8, s8c) if where == "sr" else (h8, h8c)
    assert int(hit[1, 70, 3, 2]) == 0                                      # BGR: R is the last byte
    hit_c = hit_c.clone()
    hit_c[1, 70, 3, 2] = 0
    assert torch.equal(hit, hit_c)
    other, other_c = (h8, h8c) if where == "sr" else (s8, s8c)
    assert torch.equal(other, other_c)


def test_python_entry_refuses_what_the_kernel_does_not_take():
    from srganst._abi import HipPathError
    from srganst.metrics import image_metrics_device
    x = torch.rand(1, 3, 16, 16, device="cuda")
    for sr, hr in ((x.cpu(), x), (x, x.cpu()), (x.double(), x.double()), (x.half(), x), (x, x[:, :, :12]), (x[:, :2], x[:, :2]),
                   (x[:, :, :10], x[:, :, :10]), (x[:, :, :, :10], x[:, :, :, :10]), (x[0], x[0])):
        with pytest.raises(HipPathError):
            image_metrics_device(sr, hr)
    out = image_metrics_device(x, x)
    assert out[0, 0].item() == 0.0


# ---- end to end -------------------------------------------------------------------------------------------------------------


class _Pairs(Dataset):
    """tests/test_drivers_gpu.py:_Pairs with the sizes of this file that divide by the upscale factor."""

    def __init__(self):
        from srganst.bicubic import Bicubic
        g = torch.Generator().manual_seed(9)
        self.items = []
        for h, w in ((48, 64), (72, 40), (96, 96), (212, 172)):
            gt = _smooth_hr(h, w, g)
            self.items.append((gt[0], Bicubic("cpu")(gt, scale=0.25)[0]))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _cfg(tmp, name):
    from srganst.config import Config
    cfg = Config()
    cfg.EXP.NAME = name
    cfg.EXP.N_EPOCHS = 2
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
    cfg.DATA.BATCH_SIZE = 4
    cfg.LOG_TRAIN_PERIOD = 2
    cfg.DATA.TEST_SR_IMAGES_DIR = os.path.join(tmp, "sr")
    return cfg


def test_validate_on_device_matches_the_host_pass(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from srganst.device_data import DeviceTestSet
    from srganst.model import Generator
    from srganst.validate import _validate, test as run_test
    monkeypatch.chdir(tmp_path)
    cfg = _cfg(str(tmp_path), "e2e")
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()                  # trained for nothing
    ds = _Pairs()
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    host = _validate(G, loader, cfg, on_device=False)
    line_host = capsys.readouterr().out
    dev = _validate(G, DeviceTestSet.from_dataset(ds, cfg.DEVICE), cfg, on_device=True)
    line_dev = capsys.readouterr().out
    dev_loader = _validate(G, loader, cfg, on_device=True)    # the device path takes the host loader too
    capsys.readouterr()
    cfg.DATA.VALIDATE_ON_DEVICE = True                      # ... and on_device=None follows the config switch
    dev_cfg = _validate(G, loader, cfg)
    cfg.DATA.VALIDATE_ON_DEVICE = False
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n_validate: host {host}  device {dev}  |d| {abs(host[0] - dev[0]):.3e} {abs(host[1] - dev[1]):.3e}")
    assert math.isfinite(host[0]) and 5.0 < host[0] < 60.0
    assert abs(host[0] - dev[0]) <= BOUND and abs(host[1] - dev[1]) <= BOUND
    assert dev_loader == dev and dev_cfg == dev
    assert line_host == line_dev and "[Test] | PSNR:" in line_dev

    # test(): _metrics.txt and the written images
    torch.save(G.state_dict(), tmp_path / "g.pth")
    for concat in (False, True):
        runs = {}
        for mode in (False, True):
            cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / f"sr_{int(concat)}_{int(mode)}")
            got = run_test(cfg, save_images=True, g_path=str(tmp_path / "g.pth"), concat_w_gt=concat, dataset=ds, on_device=mode)
            d = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, "e2e")
            runs[mode] = (got, open(os.path.join(d, "_metrics.txt")).read(), d)
        capsys.readouterr()
        assert runs[True][1] == runs[False][1] and runs[True][1].count(".png | PSNR:") == len(ds)
        assert abs(runs[True][0][0] - runs[False][0][0]) <= BOUND and abs(runs[True][0][1] - runs[False][0][1]) <= BOUND
        for i in range(len(ds)):
            a = np.asarray(Image.open(os.path.join(runs[True][2], f"{i}.png")))
            b = np.asarray(Image.open(os.path.join(runs[False][2], f"{i}.png")))
            h, w = ds[i][0].shape[1:]
            assert a.shape == (h, 2 * w if concat else w, 3) and np.array_equal(a, b)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_train_is_the_same_run_whichever_way_it_validates(tmp_path, monkeypatch):
    from srganst.dataset import SyntheticImageDataset
    from srganst.loss import MSELoss
    from srganst.train import train
    monkeypatch.chdir(tmp_path)
    train_ds = SyntheticImageDataset(24, hr=96, seed=1)
    for name, on_device in (("val_dev", True), ("val_host", False)):
        cfg = _cfg(str(tmp_path), name)
        cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
        cfg.SOLVER.D_UPDATE_INTERVAL = 2
        cfg.DATA.ON_DEVICE = True
        cfg.DATA.VALIDATE_ON_DEVICE = on_device
        train(cfg, train_dataset=train_ds, test_dataset=_Pairs(), max_steps_per_epoch=3)
    for f in ("g_last.pth", "d_last.pth", "g_best.pth", "d_best.pth"):
        assert os.path.exists(f"results/val_dev/{f}") and os.path.exists(f"results/val_host/{f}"), f
        a, b = _load(f"results/val_dev/{f}"), _load(f"results/val_host/{f}")
        assert _same(a, b), f"{f} differs between device and host validation"
    g_last = _load("results/val_dev/g_last.pth")
    assert int(g_last["trunk.0.rcb.1.num_batches_tracked"]) == 6             # 2 epochs x 3 steps: validation bumped nothing
    # g_best comes from ONE epoch, the same in both runs (equal files above): tell which from the files
    first_epoch_best = not _same(_load("results/val_dev/g_best.pth"), g_last)
    print("g_best is from epoch", 1 if first_epoch_best else 2)
