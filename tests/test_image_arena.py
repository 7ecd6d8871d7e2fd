"""CPU: the host side of training from whole images on the device (srganst.device_data: DeviceImageArena, DeviceCropLoader,
crops_reference; srganst.prepare_dataset) - the virtual tile list against the reference script's two range loops, the cv2-free tile
cutter, the eight transforms and their index rule, the per-epoch descriptors (seeding, sharding, the default RNG left alone), the
host-side refusals and the C-ABI entry's argument checks.  The kernel itself runs in test_image_arena_gpu.py."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler
from torch.utils.data.distributed import DistributedSampler

S, STEP = 16, 12          # small tiles: the host logic does not depend on the size (a multiple of 4, as the kernel wants)


def _images(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _grid(sizes, size, step):
    """The reference's loops (data-prep/prepare_dataset.py:34-47), restated: (image, pos_y, pos_x) in the order it writes them."""
    out = []
    for n, (h, w) in enumerate(sizes):
        if size <= h and size <= w:
            for pos_y in range(0, h - size + 1, step):
                for pos_x in range(0, w - size + 1, step):
                    out.append((n, pos_y, pos_x))
    return out


SIZES = [(S, S), (S + STEP - 1, S + STEP - 1), (S - 1, 40), (S + STEP, 2 * S + 5), (40, S - 3), (33, 47), (S, S + STEP)]


def _arena(sizes=SIZES, size=S, step=STEP, seed=0):
    from srganst.device_data import DeviceImageArena
    imgs = _images(sizes, seed)
    return imgs, DeviceImageArena.from_arrays(imgs, size, step, 4, "cpu")


def test_tile_enumeration_equals_the_reference_loops():
    from srganst.device_data import tile_grid
    for size, step in ((S, STEP), (S, S), (S, 1), (8, 24)):
        ref = _grid(SIZES, size, step)
        got = tile_grid(SIZES, size, step)
        assert got.dtype == np.int32 and got.shape == (len(ref), 3)
        assert got.tolist() == [list(r) for r in ref]
    ref = _grid(SIZES, S, STEP)
    per_image = [sum(1 for r in ref if r[0] == n) for n in range(len(SIZES))]
    assert per_image[0] == 1 and per_image[1] == 1          # exactly S, and S + step - 1: one tile each
    assert per_image[2] == 0 and per_image[4] == 0          # smaller than S on one side: skipped
    assert per_image[3] == 2 * 2 and per_image[5] == 2 * 3  # odd widths
    _, a = _arena()
    assert len(a) == len(ref) and a.tiles.tolist() == [list(r) for r in ref]
    assert a.n_images == len(SIZES)                          # the small images stay in the arena, they just hold no tile


def test_arena_layout_is_packed_and_aligned():
    imgs, a = _arena()
    assert a.arena.dtype == torch.uint8 and a.arena.numel() % 16 == 0
    end = 0
    for im, (off, h, w) in zip(imgs, a.table_host.tolist()):
        assert off % 16 == 0 and off >= end and off - end < 16 and (h, w) == im.shape[:2]
        end = off + h * w * 3
        assert np.array_equal(a.arena[off:end].numpy().reshape(h, w, 3), im)
    assert a.table.dtype == torch.int64 and a.table.shape == (len(imgs), 3)


def test_from_dir_decodes_whole_images_in_file_order(tmp_path, monkeypatch):
    from PIL import Image
    from srganst import device_data
    from srganst.dataset import TrainImageDataset, read_image_hwc
    d = tmp_path / "orig"
    d.mkdir()
    for i, im in enumerate(_images([(33, 47), (20, 21), (64, 50), (S, S), (17, 90)], seed=5)):
        Image.fromarray(im).save(d / f"im{i}.png")
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (30, 31), dtype=np.uint8), "L").save(d / "gray.png")
    monkeypatch.setattr(device_data, "_CHUNK_BYTES", 64 * 50 * 3 + 100)       # several staging groups
    a = device_data.DeviceImageArena.from_dir(str(d), S, STEP, 4, "cpu")
    files = TrainImageDataset(str(d), 4).image_file_names
    assert a.n_images == len(files) == 6
    for f, (off, h, w) in zip(files, a.table_host.tolist()):
        ref = read_image_hwc(f)
        assert ref.shape == (h, w, 3) and np.array_equal(a.arena[off:off + h * w * 3].numpy().reshape(h, w, 3), ref)
    with pytest.raises(ValueError, match="no images"):
        device_data.DeviceImageArena.from_dir(str(tmp_path / "nothing_here"), S, STEP, 4, "cpu")


def test_prepare_dataset_writes_exactly_the_reference_tiles(tmp_path):
    from PIL import Image
    from srganst import prepare_dataset
    src, dst = tmp_path / "orig", tmp_path / "train"
    src.mkdir()
    imgs = _images(SIZES, seed=2)
    names = [f"pic{i:02d}.png" for i in range(len(imgs))]
    for n, im in zip(names, imgs):
        Image.fromarray(im).save(src / n)
    prepare_dataset.main(["--input_dir", str(src), "--output_dir", str(dst), "--output_size", str(S), "--step_size", str(STEP),
                          "--num_workers", "3"])
    expected = {}
    for n, (h, w) in enumerate(SIZES):            # the reference's loops and file names, restated
        index = 1
        if S <= h and S <= w:
            for pos_y in range(0, h - S + 1, STEP):
                for pos_x in range(0, w - S + 1, STEP):
                    expected[f"{names[n].split('.')[-2]}_{index:04d}.{names[n].split('.')[-1]}"] = imgs[n][pos_y:pos_y + S, pos_x:pos_x + S]
                    index += 1
    assert sorted(os.listdir(dst)) == sorted(expected)
    for name, ref in expected.items():
        with Image.open(dst / name) as t:
            assert t.mode == "RGB" and np.array_equal(np.asarray(t), ref), name
    assert prepare_dataset.tile_name("a.b.jpeg", 12) == "b_0012.jpeg"


def test_the_eight_transforms_are_distinct_and_follow_the_index_rule():
    from srganst.device_data import crops_reference
    imgs = _images([(40, 37)], seed=3)
    y0, x0 = 5, 7
    C = torch.from_numpy(imgs[0][y0:y0 + S, x0:x0 + S].copy())                   # [S, S, 3]
    desc = [(0, y0, x0, t) for t in range(8)]
    gt, lr = crops_reference(imgs, desc, S, 4)
    assert gt.shape == (8, 3, S, S) and lr.shape == (8, 3, S // 4, S // 4) and gt.dtype == torch.float32
    assert torch.equal(gt[0], C.permute(2, 0, 1).float() / 255.0)                # t = 0: the plain slice
    for a, b in itertools.combinations(range(8), 2):
        assert not torch.equal(gt[a], gt[b]), (a, b)
    ys, xs = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    for t in range(8):
        y1 = S - 1 - ys if t & 2 else ys
        x1 = S - 1 - xs if t & 1 else xs
        sy, sx = (x1, y1) if t & 4 else (y1, x1)
        assert torch.equal(gt[t], (C[sy, sx].permute(2, 0, 1).float() / 255.0)), t
        ref = C.permute(2, 0, 1)                                                  # the torch form of the same rule
        if t & 4:
            ref = ref.transpose(1, 2)
        if t & 2:
            ref = ref.flip(1)
        if t & 1:
            ref = ref.flip(2)
        assert torch.equal(gt[t], ref.float() / 255.0), t
    from srganst.bicubic import Bicubic
    assert torch.equal(lr, Bicubic("cpu")(gt, scale=0.25))                        # lr is the bicubic of the TRANSFORMED crop
    with pytest.raises(ValueError):
        crops_reference(imgs, [(0, 40 - S + 1, 0, 0)], S, 4)


def _loader(a, B=3, sampler=None, **kw):
    from srganst.device_data import DeviceCropLoader
    return DeviceCropLoader(a, B, sampler, **kw)


def test_switches_off_gives_the_tile_grid_untransformed():
    _, a = _arena()
    order = list(reversed(range(len(a))))
    ld = _loader(a, 3, sampler=order)
    p = ld.plan()
    n = len(order) // 3 * 3
    assert p.dtype == torch.int32 and p.shape == (n, 4) and len(ld) == n // 3
    assert torch.equal(p[:, :3], torch.from_numpy(a.tiles[order[:n]])) and int(p[:, 3].abs().max()) == 0
    ld.set_epoch(5)
    assert torch.equal(ld.plan(), p)                                               # nothing is drawn: every epoch the same grid
    assert isinstance(_loader(a).sampler, RandomSampler)


@pytest.mark.parametrize("random_crop,augment", [(True, False), (False, True), (True, True)])
def test_descriptors_repeat_per_seed_and_epoch_and_differ_across_epochs(random_crop, augment):
    _, a = _arena(sizes=[(70, 90), (33, 47), (64, 41)])
    order = list(range(len(a)))
    mk = lambda seed: _loader(a, 2, sampler=order, random_crop=random_crop, augment=augment, seed=seed)
    l0, l1, l2 = mk(7), mk(7), mk(8)
    plans = []
    for epoch in range(3):
        for ld in (l0, l1, l2):
            ld.set_epoch(epoch)
        p0, p1, p2 = l0.plan(), l1.plan(), l2.plan()
        assert torch.equal(p0, p1) and torch.equal(p0, l0.plan())
        assert not torch.equal(p0, p2)                                              # another seed, another draw
        plans.append(p0)
        tiles = torch.from_numpy(a.tiles[order[: p0.shape[0]]])
        assert torch.equal(p0[:, 0], tiles[:, 0])                                   # the image of a tile never changes
        assert torch.equal(p0[:, 1:3], tiles[:, 1:]) != random_crop
        assert (int(p0[:, 3].max()) > 0) == augment and 0 <= int(p0[:, 3].min()) and int(p0[:, 3].max()) <= 7
        a.check_desc(p0.numpy())
    assert not torch.equal(plans[0], plans[1]) and not torch.equal(plans[1], plans[2])


def test_epoch_counter_advances_per_iter(monkeypatch):
    from srganst.device_data import DeviceImageArena
    _, a = _arena(sizes=[(70, 90), (33, 47)])
    seen = []
    monkeypatch.setattr(DeviceImageArena, "crops", lambda self, desc, gt, lr: seen.append(desc.clone()) or (None, None))
    order = list(range(len(a)))
    ld = _loader(a, 4, sampler=order, random_crop=True, augment=True, seed=3)
    ref = _loader(a, 4, sampler=order, random_crop=True, augment=True, seed=3)
    for epoch in range(3):
        assert ld.epoch == epoch
        seen.clear()
        n = sum(1 for _ in ld)
        assert n == len(ld) == len(seen)
        ref.set_epoch(epoch)
        assert torch.equal(torch.cat(seen), ref.plan())
    ld.set_epoch(1)
    seen.clear()
    list(ld)
    ref.set_epoch(1)
    assert torch.equal(torch.cat(seen), ref.plan()) and ld.epoch == 2


@pytest.mark.parametrize("random_crop,augment", [(False, False), (True, False), (False, True), (True, True)])
def test_two_shards_of_world_2_give_the_world_1_descriptors(random_crop, augment):
    _, a = _arena(sizes=[(70, 90), (33, 47), (64, 41), (S, S)])
    kw = dict(random_crop=random_crop, augment=augment, seed=11)
    for epoch in (0, 1):
        whole = _loader(a, 1, sampler=list(range(len(a))), **kw)
        whole.set_epoch(epoch)
        by_tile = whole.plan()                                                      # world 1: row i = tile i's descriptor
        seen = []
        for rank in (0, 1):
            smp = DistributedSampler(a, num_replicas=2, rank=rank, shuffle=True, seed=0)
            smp.set_epoch(epoch)
            ld = _loader(a, 1, sampler=smp, **kw)
            ld.set_epoch(epoch)
            idx = list(iter(smp))
            assert torch.equal(ld.plan(), by_tile[idx])                              # the same tiles give the same descriptors
            seen += idx
        assert set(seen) == set(range(len(a)))
        # ... whatever the batch size
        big = _loader(a, 5, sampler=list(range(len(a))), **kw)
        big.set_epoch(epoch)
        assert torch.equal(big.plan(), by_tile[: len(big) * 5])


@pytest.mark.parametrize("random_crop,augment", [(False, False), (True, False), (False, True), (True, True)])
def test_building_a_plan_leaves_the_default_rng_alone(random_crop, augment):
    _, a = _arena()
    torch.manual_seed(123)
    ld = _loader(a, 2, sampler=list(range(len(a))), random_crop=random_crop, augment=augment, seed=1)
    before = torch.get_rng_state()
    ld.plan()
    ld.set_epoch(3)
    ld.plan()
    assert torch.equal(torch.get_rng_state(), before)


def test_host_refusals():
    from srganst.config import Config
    from srganst.device_data import DeviceImageArena, check_switches, on_device, train_loader
    imgs, a = _arena()
    n_big = 5                                                                      # SIZES[5] = (33, 47)
    a.check_desc(np.array([[n_big, 33 - S, 47 - S, 7], [0, 0, 0, 0]]))
    for bad in ([n_big, 33 - S + 1, 0, 0], [n_big, 0, 47 - S + 1, 0], [n_big, -1, 0, 0], [n_big, 0, -1, 0], [2, 0, 0, 0],
                [len(SIZES), 0, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 8], [0, 0, 0, -1]):
        with pytest.raises(IndexError):
            a.check_desc(np.array([[0, 0, 0, 0], bad]))
    with pytest.raises(IndexError):
        _loader(a, 2, sampler=[0, 1, 2, len(a)]).plan()
    with pytest.raises(ValueError, match="tile"):
        DeviceImageArena.from_arrays(_images([(S - 1, 50), (50, S - 1)]), S, STEP, 4, "cpu")      # an empty tile list
    with pytest.raises(ValueError):
        DeviceImageArena.from_arrays([np.zeros((20, 20), np.uint8)], S, STEP, 4, "cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        DeviceImageArena.from_arrays(imgs, 18, STEP, 4, "cpu")
    with pytest.raises(ValueError):
        a.crops(torch.zeros(2, 3, dtype=torch.int32))
    for key in ("RANDOM_CROP", "AUGMENT"):
        cfg = Config()
        cfg.DATA[key] = True
        with pytest.raises(ValueError, match="ON_DEVICE_WHOLE_IMAGES"):
            check_switches(cfg)
        with pytest.raises(ValueError, match="ON_DEVICE_WHOLE_IMAGES"):
            on_device(cfg)
        cfg.DATA.ON_DEVICE = True                                                   # the pre-cut device path has no such switch either
        with pytest.raises(ValueError, match="ON_DEVICE_WHOLE_IMAGES"):
            train_loader(cfg, None, 1, 0)
        cfg.DATA.ON_DEVICE_WHOLE_IMAGES = True
        assert on_device(cfg) is True


def test_config_defaults_are_off_and_additive():
    from srganst.config import Config
    from srganst.device_data import on_device
    cfg = Config()
    assert cfg.DATA.ON_DEVICE_WHOLE_IMAGES is False and cfg.DATA.RANDOM_CROP is False and cfg.DATA.AUGMENT is False
    assert cfg.DATA.CROP_STEP == 96 and cfg.DATA.TRAIN_ORIGINAL_IMAGES_DIR == f"/work3/{cfg.EXP.USER}/data/original"
    assert on_device(cfg) is False
    cfg.DATA.ON_DEVICE = True
    assert on_device(cfg) is True


def test_train_loader_returns_the_crop_loader(tmp_path):
    from PIL import Image
    from srganst.config import Config
    from srganst.device_data import DeviceCropLoader, DeviceImageSet, train_loader
    d = tmp_path / "orig"
    d.mkdir()
    for i, im in enumerate(_images([(33, 47), (20, 21), (64, 50)], seed=5)):
        Image.fromarray(im).save(d / f"im{i}.png")
    cfg = Config()
    cfg.DEVICE = "cpu"
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES, cfg.DATA.TRAIN_ORIGINAL_IMAGES_DIR = True, str(d)
    cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP, cfg.DATA.BATCH_SIZE = S, STEP, 2
    cfg.DATA.RANDOM_CROP, cfg.DATA.AUGMENT, cfg.DATA.SEED, cfg.EXP.START_EPOCH = True, True, 4, 2
    ld, sampler = train_loader(cfg, None, 1, 0)
    assert isinstance(ld, DeviceCropLoader) and sampler is None
    assert (ld.random_crop, ld.augment, ld.seed, ld.epoch, ld.batch_size) == (True, True, 4, 2, 2)
    assert len(ld.dset) == len(_grid([(33, 47), (20, 21), (64, 50)], S, STEP)) and (ld.dset.crop, ld.dset.step) == (S, STEP)
    ld2, sampler2 = train_loader(cfg, None, 2, 1)
    assert isinstance(sampler2, DistributedSampler) and ld2.sampler is sampler2
    with pytest.raises(ValueError, match="TRAIN_ORIGINAL_IMAGES_DIR"):
        train_loader(cfg, [(torch.zeros(3, S, S), torch.zeros(3, 4, 4))], 1, 0)
    assert not isinstance(ld.dset, DeviceImageSet)


def test_span_bounds_every_band():
    """The LDS bound handed to the kernel: no band's tap rows (and own rows) extend over more consecutive crop rows."""
    from srganst.bicubic import Bicubic
    from srganst.device_data import DeviceImageArena
    for size, up in ((96, 4), (96, 2), (192, 4), (192, 2), (64, 8)):
        a = DeviceImageArena.from_arrays(_images([(size, size + 1)]), size, size, up, "cpu")
        _, iy, _, _ = Bicubic("cpu").tables(size, size, 1.0 / up, "cpu")
        o = size // up
        need = 0
        for band in range(o):
            rows = set(iy[band].tolist()) | set(range(band * size // o, (band + 1) * size // o))
            need = max(need, max(rows) - min(rows) + 1)
        assert a.span(True, True) == need and a.span(False, True) <= need and a.span(True, False) == 4
        assert need <= iy.shape[1] + size // o


def test_crops_entry_is_exported_and_checks_its_arguments_on_the_host():
    from srganst import _abi
    assert "sst_gather_crops" in _abi.SIGNATURES
    lib = _abi.lib()
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "sst_gather_crops")
    rc = lib.sst_gather_crops(None, 16, None, 1, None, 1, 96, None, None, None, None, None, None, None, 24, 24, 16, 16, 16, None)
    assert rc != 0 and b"sst_gather_crops" in lib.sst_last_error()
    _, a = _arena()
    with pytest.raises(_abi.HipPathError):                                         # no CPU fallback
        a.crops(torch.zeros(2, 4, dtype=torch.int32))
