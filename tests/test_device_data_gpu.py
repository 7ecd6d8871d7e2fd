"""GPU: the HBM-resident training set (srganst.device_data, csrc/data.hip: sst_gather_batch) against the host data path - the
gather kernel against host-stacked batches and Bicubic, from_dir against TrainImageDataset, a TrainEngine fed by DeviceLoader against
one fed host batches of the same indices (bit for bit), and the warmup()/train() drivers with DATA.ON_DEVICE."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler

pytestmark = pytest.mark.gpu


def _within_host_bound(a, b):
    """Device LR against the CPU Bicubic of the data loader: equal on the 1/255 grid except where 255*x lands within float rounding
    of a half-way point (summation order differs) - the bound of test_drivers_gpu.test_bicubic_on_device_matches_reference_golden."""
    return float((a - b).abs().max()) <= 1.0 / 255 + 1e-7 and float((a != b).float().mean()) < 1e-3


@pytest.mark.parametrize("B", [1, 16, 37])
@pytest.mark.parametrize("hw", [(96, 96), (192, 192), (64, 96)])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_gather_kernel_matches_host_path(B, hw, s):
    from srganst.bicubic import Bicubic
    from srganst.device_data import DeviceImageSet
    H, W = hw
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + s)
    N = 23
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    dset = DeviceImageSet(u8.cuda(), s)
    idx = torch.randint(0, N, (B,), generator=g)
    idx[B // 2] = idx[0]                                                  # repeats allowed
    gt, lr = dset.batch(idx.to(torch.int32).cuda())
    torch.cuda.synchronize()
    ref = u8[idx].permute(0, 3, 1, 2).float() / 255.0
    assert gt.shape == (B, 3, H, W) and lr.shape == (B, 3, H // s, W // s)
    assert torch.equal(gt.cpu(), ref)
    lr_dev = Bicubic("cuda")(ref.cuda(), scale=1.0 / s)
    assert torch.equal(lr, lr_dev)
    assert _within_host_bound(lr.cpu(), Bicubic("cpu")(ref, scale=1.0 / s))
    # one output only, and into given buffers
    gt2, none = dset.batch(idx.to(torch.int32).cuda(), with_lr=False)
    none2, lr2 = dset.batch(idx.to(torch.int32).cuda(), lr_out=torch.full_like(lr, 7.0), with_gt=False)
    assert none is None and none2 is None
    assert torch.equal(gt2, gt) and torch.equal(lr2, lr)


def test_from_dir_matches_train_image_dataset(tmp_path):
    from PIL import Image
    from srganst.dataset import TrainImageDataset
    from srganst.device_data import DeviceImageSet
    rng = np.random.default_rng(3)
    for i in range(7):
        Image.fromarray(rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)).save(tmp_path / f"c{i}.png")
    Image.fromarray(rng.integers(0, 256, (96, 96, 4), dtype=np.uint8), "RGBA").save(tmp_path / "rgba.png")
    Image.fromarray(rng.integers(0, 256, (96, 96), dtype=np.uint8), "L").save(tmp_path / "gray.png")
    ds = TrainImageDataset(str(tmp_path), 4)
    dset = DeviceImageSet.from_dir(str(tmp_path), 4, "cuda")
    idx = [8, 0, 3, 3, 7, 1]
    gt, lr = dset.batch(torch.tensor(idx, dtype=torch.int32, device="cuda"))
    ref_gt = torch.stack([ds[i][0] for i in idx])
    ref_lr = torch.stack([ds[i][1] for i in idx])
    assert torch.equal(gt.cpu(), ref_gt)
    assert _within_host_bound(lr.cpu(), ref_lr)


def _narrow_cfg():
    from srganst.config import Config
    from srganst.loss import MSELoss, StructureTensorLoss
    cfg = Config()
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
    cfg.SOLVER.D_UPDATE_INTERVAL = 2
    return cfg


def test_engine_fed_by_device_loader_equals_host_batches():
    """Same weights, same indices: DeviceLoader with the engine's buffers bound against host-stacked batches + Bicubic("cuda"),
    six graphed steps; parameters, BatchNorm buffers and per-step losses bit for bit (narrow model: reproducible by construction)."""
    from srganst.bicubic import Bicubic
    from srganst.dataset import SyntheticImageDataset
    from srganst.device_data import DeviceImageSet, DeviceLoader
    from srganst.engine import TrainEngine
    from srganst.model import Discriminator, Generator
    ds = SyntheticImageDataset(24, hr=96, seed=3)
    dset = DeviceImageSet.from_dataset(ds, 4, "cuda")
    sampler = lambda: RandomSampler(dset, generator=torch.Generator().manual_seed(11))

    def run(device_fed):
        cfg = _narrow_cfg()
        torch.manual_seed(1)
        D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
        eng = TrainEngine(cfg, G, D, use_graph=True, adam_capturable=True)
        losses = []
        if device_fed:
            loader = DeviceLoader(dset, 4, sampler())
            assert len(loader) == 6
            for gt, lr in loader:
                eng.step(gt, lr)
                loader.bind(eng.gt, eng.lr)
                losses.append({k: v.clone() for k, v in eng.loss_values.items()})
            assert eng.gt.data_ptr() == gt.data_ptr() and eng.lr.data_ptr() == lr.data_ptr()   # the last batch landed in place
        else:
            plan = DeviceLoader(dset, 4, sampler()).plan().view(6, 4)
            for k in range(6):
                gt = torch.stack([ds[int(i)][0] for i in plan[k]]).cuda()
                eng.step(gt, Bicubic("cuda")(gt, scale=0.25))
                losses.append({k2: v.clone() for k2, v in eng.loss_values.items()})
        torch.cuda.synchronize()
        out = (G.state_dict(), D.state_dict(), losses)
        eng.close()
        return out

    g1, d1, l1 = run(True)
    g2, d2, l2 = run(False)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in d1:
        assert torch.equal(d1[k], d2[k]), k
    assert len(l1) == len(l2) == 6
    for a, b in zip(l1, l2):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_drivers_on_device(tmp_path, monkeypatch):
    from srganst.dataset import SyntheticImageDataset
    from srganst.loss import MSELoss, StructureTensorLoss
    from srganst.train import train
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs, _cfg
    monkeypatch.chdir(tmp_path)
    train_ds = SyntheticImageDataset(24, hr=96, seed=1)
    cfg = _cfg(str(tmp_path), "warm_dev")
    cfg.DATA.ON_DEVICE = True
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss(), "ST": StructureTensorLoss()}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0, "ST": 1 / 3}
    warmup(cfg, train_dataset=train_ds, test_dataset=_Pairs(), max_steps_per_epoch=5)
    sd = torch.load("results/warm_dev/g_last.pth", map_location="cpu", weights_only=True)
    assert int(sd["trunk.0.rcb.1.num_batches_tracked"]) == 10                  # 2 epochs x 5 steps
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())

    cfg2 = _cfg(str(tmp_path), "gan_dev")
    cfg2.DATA.ON_DEVICE = True
    cfg2.MODEL.G_CONTINUE_FROM_WARMUP = True
    cfg2.MODEL.G_WARMUP_WEIGHTS = "results/warm_dev/g_last.pth"
    cfg2.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg2.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
    cfg2.SOLVER.D_UPDATE_INTERVAL = 2
    train(cfg2, train_dataset=train_ds, test_dataset=_Pairs(), max_steps_per_epoch=5)
    for f in ("g_last.pth", "d_last.pth"):
        assert os.path.exists(os.path.join("results/gan_dev", f))
    dsd = torch.load("results/gan_dev/d_last.pth", map_location="cpu", weights_only=True)
    assert int(dsd["features.3.num_batches_tracked"]) > 0
    gsd = torch.load("results/gan_dev/g_last.pth", map_location="cpu", weights_only=True)
    assert int(gsd["trunk.0.rcb.1.num_batches_tracked"]) > 10                  # past the warm start's 10
