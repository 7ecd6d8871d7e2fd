"""CPU: the host side of the HBM-resident training set (srganst.device_data) - threaded decode against the host loader's
read_image, refusal of mixed crop sizes and off-grid sets, the 1/255 LUT, the per-epoch index plan of DeviceLoader, and the C-ABI
entry's host-side argument checks.  The gather kernel itself runs in test_device_data_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.utils.data import Dataset, RandomSampler
from torch.utils.data.distributed import DistributedSampler


def _write_pngs(d, n, h=24, w=32, seed=0):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"rgb_{i:03d}.png"))
    Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA").save(os.path.join(d, "rgba.png"))
    Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L").save(os.path.join(d, "gray.png"))


class _Grid(Dataset):
    def __init__(self, n=10, hr=16, off_grid_item=None):
        g = torch.Generator().manual_seed(4)
        self.u8 = torch.randint(0, 256, (n, 3, hr, hr), generator=g, dtype=torch.uint8)
        self.off = off_grid_item

    def __len__(self):
        return self.u8.shape[0]

    def __getitem__(self, i):
        gt = self.u8[i].float() / 255
        if i == self.off:
            gt = gt.clone()
            gt[1, 2, 3] += 1e-4
        return gt, gt[:, ::4, ::4]


def test_threaded_decode_matches_read_image_in_file_order(tmp_path, monkeypatch):
    from srganst import device_data
    from srganst.dataset import TrainImageDataset, read_image
    d = str(tmp_path / "crops")
    _write_pngs(d, 9)
    monkeypatch.setattr(device_data, "_CHUNK_BYTES", 3 * 24 * 32 * 3)      # several staging chunks, the last one partial
    s = device_data.DeviceImageSet.from_dir(d, 4, "cpu")
    files = TrainImageDataset(d, 4).image_file_names
    ref = torch.stack([read_image(f) for f in files]).permute(0, 2, 3, 1)
    assert len(s) == len(files) == 11 and s.store.shape == (11, 24, 32, 3) and s.store.dtype == torch.uint8
    assert torch.equal(s.store, ref)
    assert (s.H, s.W, s.oh, s.ow) == (24, 32, 6, 8)


def test_mixed_crop_sizes_are_refused_with_the_file_named(tmp_path):
    from PIL import Image
    from srganst.device_data import DeviceImageSet
    from srganst.dataset import TrainImageDataset
    d = str(tmp_path / "crops")
    _write_pngs(d, 4)
    Image.fromarray(np.zeros((24, 40, 3), np.uint8)).save(os.path.join(d, "odd_one.png"))
    files = TrainImageDataset(d, 4).image_file_names
    size = lambda f: Image.open(f).size
    first_bad = next(f for f in files[1:] if size(f) != size(files[0]))     # the odd file, or the file after it if it is listed first
    with pytest.raises(ValueError, match=os.path.basename(first_bad)):
        DeviceImageSet.from_dir(d, 4, "cpu")


def test_from_dataset_rebuilds_the_store_and_refuses_off_grid_gt():
    from srganst.device_data import DeviceImageSet
    ds = _Grid()
    s = DeviceImageSet.from_dataset(ds, 4, "cpu")
    assert torch.equal(s.store, ds.u8.permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match="1/255 grid"):
        DeviceImageSet.from_dataset(_Grid(off_grid_item=7), 4, "cpu")


def test_lut_is_u8_over_255():
    from srganst.device_data import lut
    u8 = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(lut("cpu"), u8.float() / 255.0)
    assert torch.equal(lut("cpu")[u8.long()], u8.float() / 255.0)


def test_epoch_plan_semantics():
    from srganst.device_data import DeviceImageSet, DeviceLoader
    s = DeviceImageSet.from_dataset(_Grid(n=10), 4, "cpu")
    ld = DeviceLoader(s, 3)
    assert isinstance(ld.sampler, RandomSampler) and len(ld) == 3
    p = ld.plan()
    assert p.dtype == torch.int64 and p.numel() == 9 and len(set(p.tolist())) == 9 and 0 <= int(p.min()) and int(p.max()) < 10
    # the same seeded generator gives the same plan, epoch after epoch
    a = DeviceLoader(s, 3, RandomSampler(s, generator=torch.Generator().manual_seed(5)))
    b = DeviceLoader(s, 3, RandomSampler(s, generator=torch.Generator().manual_seed(5)))
    for _ in range(2):
        assert torch.equal(a.plan(), b.plan())
    # data parallel: world 2, each rank half the set, disjoint plans; set_epoch changes the order and keeps the ranks disjoint
    for epoch in (0, 1):
        plans = []
        for rank in (0, 1):
            smp = DistributedSampler(s, num_replicas=2, rank=rank, shuffle=True, seed=0)
            smp.set_epoch(epoch)
            ld = DeviceLoader(s, 2, smp)
            assert len(ld) == 2
            plans.append(set(ld.plan().tolist()))
            assert len(plans[-1]) == 4
        assert not (plans[0] & plans[1])
    s0, s1 = DistributedSampler(s, 2, 0, shuffle=True), DistributedSampler(s, 2, 0, shuffle=True)
    s1.set_epoch(1)
    assert DeviceLoader(s, 5, s0).plan().tolist() != DeviceLoader(s, 5, s1).plan().tolist()


def test_plan_refuses_indices_outside_the_set():
    from srganst.device_data import DeviceImageSet, DeviceLoader
    s = DeviceImageSet.from_dataset(_Grid(n=4), 4, "cpu")
    with pytest.raises(IndexError):
        DeviceLoader(s, 2, sampler=[0, 1, 2, 4]).plan()


def test_batch_needs_the_device():
    from srganst import _abi
    from srganst.device_data import DeviceImageSet
    s = DeviceImageSet.from_dataset(_Grid(n=4), 4, "cpu")
    with pytest.raises(_abi.HipPathError):
        s.batch(torch.zeros(2, dtype=torch.int32))


def test_gather_entry_is_exported_and_checks_its_arguments_on_the_host():
    from srganst import _abi
    from srganst.config import Config
    assert "sst_gather_batch" in _abi.SIGNATURES
    lib = _abi.lib()
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "sst_gather_batch")
    rc = lib.sst_gather_batch(None, 1, None, 1, 96, 96, None, None, None, None, None, None, None, 24, 24, 16, 16, None)
    assert rc != 0 and b"sst_gather_batch" in lib.sst_last_error()
    assert Config().DATA.ON_DEVICE is False
