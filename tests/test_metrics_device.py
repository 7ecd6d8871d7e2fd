"""CPU: the host-side surface of device validation - the sst_image_metrics ABI entries' argument checks (made before any launch, so
safe without a GPU), DeviceTestSet against the DataLoader it replaces, the config switch, psnr_from_mse."""
import ctypes
import math

import pytest
import torch
from torch.utils.data import DataLoader, Dataset


class _Pairs(Dataset):
    """(hr [3,H,W], lr [3,H/4,W/4]) of different sizes on the 1/255 grid."""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.items = []
        for h, w in ((48, 64), (72, 40), (12, 16)):
            hr = torch.randint(0, 256, (3, h, w), generator=g).float() / 255.0
            lr = torch.randint(0, 256, (3, h // 4, w // 4), generator=g).float() / 255.0
            self.items.append((hr, lr))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _ws(lib, B, H, W):
    n = ctypes.c_int64()
    assert lib.sst_image_metrics_workspace(B, H, W, ctypes.byref(n)) == 0
    return n.value


def test_workspace_query_grows_with_the_tile_count():
    from srganst import _abi
    lib = _abi.lib()
    tiles = lambda B, H, W: B * ((H + 31) // 32) * ((W + 31) // 32)
    shapes = [(1, 11, 11), (1, 32, 32), (1, 33, 32), (1, 211, 173), (3, 96, 96), (1, 768, 1024), (2, 768, 1024)]
    sizes = [_ws(lib, *s) for s in shapes]
    assert all(n > 0 for n in sizes)
    for (sa, na) in zip(shapes, sizes):
        for (sb, nb) in zip(shapes, sizes):
            if tiles(*sa) < tiles(*sb):
                assert na < nb, (sa, na, sb, nb)
            elif tiles(*sa) == tiles(*sb):
                assert na == nb, (sa, na, sb, nb)
    n = ctypes.c_int64()
    assert lib.sst_image_metrics_workspace(0, 32, 32, ctypes.byref(n)) != 0
    assert lib.sst_image_metrics_workspace(1, 32, 32, None) != 0


def test_null_pointers_are_refused_before_any_launch():
    from srganst import _abi
    lib = _abi.lib()
    rc = lib.sst_image_metrics(None, None, 1, 32, 32, None, None, None, None, None)
    assert rc != 0 and b"null pointer" in lib.sst_last_error()
    fake = 0x1000           # never dereferenced: the check that fails comes before the launch
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        sr, hr, out, ws = args
        rc = lib.sst_image_metrics(sr, hr, 1, 32, 32, out, None, None, ws, None)
        assert rc != 0 and b"null pointer" in lib.sst_last_error(), args


@pytest.mark.parametrize("H,W", [(10, 32), (32, 10), (10, 10), (0, 32)])
def test_images_below_the_window_are_refused(H, W):
    from srganst import _abi
    lib = _abi.lib()
    fake = 0x1000           # never dereferenced: the size check comes before the launch
    rc = lib.sst_image_metrics(fake, fake, 1, H, W, fake, None, None, fake, None)
    msg = lib.sst_last_error()
    assert rc != 0 and b"11-px minimum" in msg, msg


def test_python_entry_refuses_cpu_tensors_and_bad_shapes():
    from srganst._abi import HipPathError
    from srganst.metrics import image_metrics_device
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(HipPathError):
        image_metrics_device(x, x)


def test_device_test_set_yields_what_the_loader_yields():
    from srganst.device_data import DeviceTestSet
    ds = _Pairs()
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    dset = DeviceTestSet.from_dataset(ds, "cpu")
    assert len(dset) == len(loader) == 3
    for _ in range(2):                                   # iterable again and again, like the loader
        n = 0
        for (hr_a, lr_a), (hr_b, lr_b) in zip(dset, loader):
            assert hr_a.dtype == hr_b.dtype and hr_a.shape == hr_b.shape and torch.equal(hr_a, hr_b)
            assert lr_a.dtype == lr_b.dtype and lr_a.shape == lr_b.shape and torch.equal(lr_a, lr_b)
            n += 1
        assert n == 3
    with pytest.raises(ValueError):
        DeviceTestSet([])


def test_device_test_set_leaves_the_default_generator_where_the_loader_leaves_it():
    """A DataLoader draws its base seed from the default generator per pass; the training sampler's next shuffle depends on it, so
    the device set must make the same draw for a run to be the same whichever way it validates."""
    from srganst.device_data import DeviceTestSet
    ds = _Pairs()
    torch.manual_seed(11)
    for _ in DataLoader(ds, batch_size=1, shuffle=False, num_workers=0):
        pass
    a = torch.randperm(50)
    torch.manual_seed(11)
    for _ in DeviceTestSet.from_dataset(ds, "cpu"):
        pass
    assert torch.equal(a, torch.randperm(50))


def test_device_test_set_from_dir_follows_the_test_dataset(tmp_path):
    import numpy as np
    from PIL import Image
    from srganst.dataset import TestImageDataset
    from srganst.device_data import DeviceTestSet
    rng = np.random.default_rng(0)
    for sub, sizes in (("gt", ((24, 32), (40, 20))), ("lr", ((6, 8), (10, 5)))):
        (tmp_path / sub).mkdir()
        for k, (h, w) in enumerate(sizes):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / sub / f"img{k}.png")
    ds = TestImageDataset(str(tmp_path / "gt"), str(tmp_path / "lr"))
    dset = DeviceTestSet.from_dir(str(tmp_path / "gt"), str(tmp_path / "lr"), "cpu")
    assert len(dset) == 2
    for (hr, lr), (hr_b, lr_b) in zip(dset, DataLoader(ds, batch_size=1)):
        assert torch.equal(hr, hr_b) and torch.equal(lr, lr_b)


def test_switch_defaults_to_the_host_path():
    from srganst.config import Config
    assert Config().DATA.VALIDATE_ON_DEVICE is False


def test_psnr_from_mse_follows_the_host_rule():
    import numpy as np
    from srganst.metrics import psnr_from_mse
    from srganst.utils import PSNR
    assert psnr_from_mse(0) == float("inf") and psnr_from_mse(0.0) == float("inf")
    a = np.array([[16.0, 40.5], [200.25, 90.0]])
    b = np.array([[17.0, 38.5], [190.0, 90.0]])
    assert psnr_from_mse(np.mean((a - b) ** 2)) == PSNR(a, b)
    assert psnr_from_mse(1.0) == 20 * math.log10(255.0)
    assert math.isnan(psnr_from_mse(float("nan")))
