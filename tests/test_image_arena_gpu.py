"""GPU: training batches cut from whole images on the device (srganst.device_data: DeviceImageArena / DeviceCropLoader, csrc/data.hip:
sst_gather_crops) - the kernel against crops_reference for every transform, window position, size and batch, its NaN convention,
the equivalence of the switch-less loader with DeviceLoader over tiles cut by srganst.prepare_dataset, and the train() driver with
DATA.ON_DEVICE_WHOLE_IMAGES against DATA.ON_DEVICE on those tiles (checkpoints bit for bit)."""
import math
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import Dataset, RandomSampler

pytestmark = pytest.mark.gpu


def _within_host_bound(a, b):
    """The host-versus-device bound of tests/test_device_data_gpu.py for the old kernel, taken from there unchanged: equal on the
    1/255 grid except where 255*x lands within float rounding of a half-way point (summation order differs)."""
    return float((a - b).abs().max()) <= 1.0 / 255 + 1e-7 and float((a != b).float().mean()) < 1e-3


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _sizes(S):
    return [(S, S), (S + 41, 2 * S + 13), (2 * S + 7, S + 30), (S + 5, S + 128)]          # all different, odd widths among them


def _descriptors(sizes, S, B):
    """B descriptors that walk all eight t (from t = 0) and these windows: (0, 0), x0 odd, x0 = W - S, y0 = H - S, both at once,
    an unaligned interior one, and the image that is exactly S x S."""
    def windows(n):
        h, w = sizes[n]
        return [(n, 0, 0), (n, 3, 7), (n, 1, w - S), (n, h - S, 2), (n, h - S, w - S), (n, (h - S) // 2, ((w - S) // 2) | 1)]
    wins = windows(1) + windows(2) + windows(3) + [(0, 0, 0)]
    return [(*wins[(5 * k) % len(wins)], k % 8) for k in range(B)]


@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("up", [4, 2])
@pytest.mark.parametrize("S", [96, 192])
def test_crop_kernel_matches_crops_reference(S, up, B):
    from srganst.bicubic import Bicubic
    from srganst.device_data import DeviceImageArena, crops_reference
    sizes = _sizes(S)
    imgs = _images(sizes, seed=S + up)
    arena = DeviceImageArena.from_arrays(imgs, S, S, up, "cuda")
    # B = 16: one launch over all eight t, twice, with 16 different windows; B = 1: eight launches of one sample, one per t
    batches = [_descriptors(sizes, S, 16)] if B == 16 else [[d] for d in _descriptors(sizes, S, 8)]
    assert sorted({d[3] for batch in batches for d in batch}) == list(range(8))
    for batch in batches:
        arena.check_desc(batch)
        desc = torch.tensor(batch, dtype=torch.int32, device="cuda")
        gt, lr = arena.crops(desc)
        torch.cuda.synchronize()
        ref_gt, ref_lr = crops_reference(imgs, batch, S, up)
        assert gt.shape == (len(batch), 3, S, S) and lr.shape == (len(batch), 3, S // up, S // up)
        assert torch.equal(gt.cpu(), ref_gt), batch
        assert torch.equal(lr, Bicubic("cuda")(gt, scale=1.0 / up)), batch
        assert _within_host_bound(lr.cpu(), ref_lr), batch
        # one output only, and into given buffers
        gt2, none = arena.crops(desc, with_lr=False)
        none2, lr2 = arena.crops(desc, lr_out=torch.full_like(lr, 7.0), with_gt=False)
        assert none is None and none2 is None
        assert torch.equal(gt2, gt) and torch.equal(lr2, lr)


def test_descriptor_out_of_range_yields_nan_for_that_sample_only():
    """The host checks every descriptor (check_desc); one that reaches the kernel anyway gives NaN, as in sst_gather_batch."""
    from srganst.device_data import DeviceImageArena, crops_reference
    S = 96
    sizes = _sizes(S)
    imgs = _images(sizes, seed=1)
    arena = DeviceImageArena.from_arrays(imgs, S, S, 4, "cuda")
    h, w = sizes[1]
    good = [(1, 3, 5, 6), (2, 0, 1, 1)]
    bad = [(len(sizes), 0, 0, 0), (-1, 0, 0, 0), (1, h - S + 1, 0, 0), (1, 0, w - S + 1, 0), (1, -1, 0, 0), (1, 0, -2, 0),
           (1, 0, 0, 8), (1, 0, 0, -1), (0, 0, 1, 0)]
    for d in bad:
        with pytest.raises(IndexError):
            arena.check_desc([d])
    batch = [good[0]] + bad + [good[1]]
    gt, lr = arena.crops(torch.tensor(batch, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    ref_gt, _ = crops_reference(imgs, good, S, 4)
    assert torch.equal(gt[0].cpu(), ref_gt[0]) and torch.equal(gt[-1].cpu(), ref_gt[1])
    assert bool(torch.isfinite(lr[0]).all()) and bool(torch.isfinite(lr[-1]).all())
    assert bool(torch.isnan(gt[1:-1]).all()) and bool(torch.isnan(lr[1:-1]).all())


def _write_originals(d, sizes, seed):
    """DIV2K-like whole images (smooth, on the 1/255 grid by construction) as PNGs; returns the file names."""
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    for i, (h, w) in enumerate(sizes):
        base = torch.rand(1, 3, max(h // 8, 2), max(w // 8, 2), generator=g)
        x = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)
        Image.fromarray(np.ascontiguousarray(torch.round(x[0] * 255).to(torch.uint8).permute(1, 2, 0).numpy())).save(
            os.path.join(d, f"img{i:02d}.png"))


def _cut(tmp_path, sizes, S, step, seed):
    """Whole images in <tmp>/orig, their tiles cut by srganst.prepare_dataset in <tmp>/train.  Returns (orig dir, tile dir, the tile
    files in the order of the virtual tile list: images in TrainImageDataset's file order, tiles by their index)."""
    from srganst import prepare_dataset
    from srganst.dataset import TrainImageDataset
    orig, tiles = str(tmp_path / "orig"), str(tmp_path / "train")
    _write_originals(orig, sizes, seed)
    n = prepare_dataset.prepare(orig, tiles, S, step, num_workers=4)
    ordered = []
    for f in TrainImageDataset(orig, 4).image_file_names:
        stem = os.path.basename(f).split(".")[-2]
        ordered += sorted(os.path.join(tiles, t) for t in os.listdir(tiles) if re.fullmatch(re.escape(stem) + r"_\d{4}\.png", t))
    assert len(ordered) == n == len(os.listdir(tiles))
    return orig, tiles, ordered


SIZES_E2E = [(96, 96), (200, 301), (150, 197), (96, 250), (300, 120), (90, 400)]     # 1 + 6 + 2 + 2 + 3 + 0 = 14 tiles


def test_switches_off_equals_device_loader_over_tiles_cut_by_prepare_dataset(tmp_path):
    """The same images, as tiles cut by prepare_dataset in a DeviceImageSet and whole in a DeviceImageArena: the same sampler seed
    gives the same batches over a whole epoch.  DeviceImageSet.from_dir lists the tile directory in the file system's order, the
    arena's tiles are in the reference script's order; the sampler draws tile numbers of the latter and `pos` translates them to
    the former's positions (an index translation only: both loaders see the same draw of the same generator)."""
    from srganst.dataset import TrainImageDataset
    from srganst.device_data import DeviceCropLoader, DeviceImageArena, DeviceImageSet, DeviceLoader
    S, B = 96, 4
    orig, tiles, ordered = _cut(tmp_path, SIZES_E2E, S, 48, seed=5)
    dset = DeviceImageSet.from_dir(tiles, 4, "cuda")
    arena = DeviceImageArena.from_dir(orig, S, 48, 4, "cuda")
    assert len(dset) == len(arena) == len(ordered) > 3 * B
    listed = TrainImageDataset(tiles, 4).image_file_names
    pos = [listed.index(f) for f in ordered]                                       # virtual tile number -> position in the store
    for seed in (3, 4):
        draw = list(RandomSampler(arena, generator=torch.Generator().manual_seed(seed)))
        old = DeviceLoader(dset, B, sampler=[pos[v] for v in draw])
        new = DeviceCropLoader(arena, B, sampler=RandomSampler(arena, generator=torch.Generator().manual_seed(seed)))
        assert len(old) == len(new) == len(ordered) // B
        n = 0
        for (gt0, lr0), (gt1, lr1) in zip(old, new):
            assert torch.equal(gt0, gt1) and torch.equal(lr0, lr1)
            n += 1
        assert n == len(new)


class _Tiles(Dataset):
    """The pre-cut tiles as a (gt, lr) dataset in a given file order (TrainImageDataset's items)."""

    def __init__(self, files):
        from srganst.bicubic import Bicubic
        self.files, self.bicubic = files, Bicubic("cpu")

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from srganst.dataset import read_image
        gt = read_image(self.files[i]).float().unsqueeze(0) / 255.0
        return gt.squeeze(0), self.bicubic(gt, scale=0.25).squeeze(0)


def _train_cfg(tmp, name):
    from srganst.loss import MSELoss, StructureTensorLoss
    from test_drivers_gpu import _cfg
    cfg = _cfg(tmp, name)
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
    cfg.SOLVER.D_UPDATE_INTERVAL = 2
    cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 96, 96
    return cfg


def _checkpoints(name):
    return {f: torch.load(os.path.join("results", name, f), map_location="cpu", weights_only=True) for f in ("g_last.pth", "d_last.pth")}


def test_train_from_whole_images_equals_train_from_the_cut_tiles(tmp_path, monkeypatch):
    from srganst.train import train
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    orig, tiles, ordered = _cut(tmp_path, SIZES_E2E, 96, 96, seed=6)
    assert len(ordered) == 14

    cfg = _train_cfg(str(tmp_path), "gan_tiles")
    cfg.DATA.ON_DEVICE = True
    train(cfg, train_dataset=_Tiles(ordered), test_dataset=_Pairs(), max_steps_per_epoch=3)

    cfg = _train_cfg(str(tmp_path), "gan_whole")
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
    cfg.DATA.TRAIN_ORIGINAL_IMAGES_DIR = orig
    train(cfg, test_dataset=_Pairs(), max_steps_per_epoch=3)

    a, b = _checkpoints("gan_tiles"), _checkpoints("gan_whole")
    for f in a:
        assert a[f].keys() == b[f].keys()
        for k in a[f]:
            assert torch.equal(a[f][k], b[f][k]), (f, k)
    assert int(a["g_last.pth"]["trunk.0.rcb.1.num_batches_tracked"]) == 6           # 2 epochs x 3 steps


def test_random_crop_and_augment_run_is_finite_and_repeats(tmp_path, monkeypatch, capsys):
    from srganst.train import train
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    orig = str(tmp_path / "orig")
    _write_originals(orig, SIZES_E2E, seed=7)
    sds = []
    for name in ("aug_a", "aug_b"):
        cfg = _train_cfg(str(tmp_path), name)
        cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = True
        cfg.DATA.TRAIN_ORIGINAL_IMAGES_DIR = orig
        train(cfg, test_dataset=_Pairs(), max_steps_per_epoch=3)
        out = capsys.readouterr().out
        losses = [float(m) for m in re.findall(r"\[(?:D|G) loss: ([^\]]+)\]", out)]
        assert len(losses) >= 4 and all(math.isfinite(v) for v in losses), out
        sds.append(_checkpoints(name))
    for f in sds[0]:
        for k, v in sds[0][f].items():
            assert torch.equal(v, sds[1][f][k]), (f, k)
            assert not v.is_floating_point() or bool(torch.isfinite(v).all()), (f, k)
    # and the switches do change the data: not the grid run's weights
    cfg = _train_cfg(str(tmp_path), "grid")
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
    cfg.DATA.TRAIN_ORIGINAL_IMAGES_DIR = orig
    train(cfg, test_dataset=_Pairs(), max_steps_per_epoch=3)
    grid = _checkpoints("grid")
    assert any(not torch.equal(v, grid["g_last.pth"][k]) for k, v in sds[0]["g_last.pth"].items())
