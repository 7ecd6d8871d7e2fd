"""Training batches from an HBM-resident image set (config.DATA.ON_DEVICE).

The prepared HR crops are decoded ONCE and kept on the device as uint8 [N, H, W, 3] (HWC/RGB, as read_image decodes them); each
training batch is then ONE HIP launch (csrc/data.hip: sst_gather_batch) that gathers the batch's crops by index, converts them to
fp32 NCHW on the 1/255 grid and synthesises the x1/upscale bicubic LR in the same pass - the values TrainImageDataset + the
default collate produce (gt bit for bit; lr bit for bit with Bicubic("cuda")(gt), within the host-versus-device bound of the CPU
Bicubic).  No decode, no host-to-device copy and no sync per step.  The cost: the whole HR set in device memory on every rank.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch import Tensor

from . import _abi
from .bicubic import Bicubic
from .dataset import TestImageDataset, TrainImageDataset, read_image_hwc

_CHUNK_BYTES = 64 << 20          # host staging: decoded crops go to the device in pinned chunks of at most this size
_MARGIN_BYTES = 2 << 30          # device memory left to the training step when the set is sized against mem_get_info


def lut(device) -> Tensor:
    """float(u) / 255 for u = 0..255, made by torch on the host: gt = lut[u8] is bit-identical to u8.float() / 255."""
    return (torch.arange(256, dtype=torch.uint8).float() / 255.0).to(device)


def decode_threads() -> int:
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _check_fits(nbytes: int, device: torch.device) -> None:
    if device.type != "cuda":
        return
    free, _ = torch.cuda.mem_get_info(device)
    if nbytes > free - _MARGIN_BYTES:
        raise MemoryError(f"DeviceImageSet: the image set needs {nbytes} bytes of device memory, {free} bytes are free on {device} "
                          f"and {_MARGIN_BYTES} are kept for training; use the host loader (DATA.ON_DEVICE = False)")


class DeviceImageSet:
    """The HR crops of a training set as one uint8 [N, H, W, 3] tensor on one device; batch() makes (gt, lr) batches from it."""

    def __init__(self, store: Tensor, upscale: int):
        if store.dtype != torch.uint8 or store.dim() != 4 or store.shape[3] != 3:
            raise ValueError(f"DeviceImageSet: store must be uint8 [N, H, W, 3], got {store.dtype} {tuple(store.shape)}")
        self.store = store.contiguous()
        self.upscale = int(upscale)
        self.device = store.device
        self.lut = lut(self.device)
        _, self.H, self.W, _ = store.shape
        self.oh, self.ow = int(self.H * (1.0 / self.upscale)), int(self.W * (1.0 / self.upscale))
        self._bicubic = Bicubic(str(self.device))

    def __len__(self) -> int:
        return self.store.shape[0]

    @classmethod
    def from_dir(cls, gt_dir: str, upscale: int, device) -> "DeviceImageSet":
        """Decode every crop of `gt_dir` (TrainImageDataset's file list and order) with a thread pool, chunk by chunk through a
        pinned staging buffer; the whole set is never held in host memory.  Threads, not processes: a process that has
        initialised HIP must not fork decoders (utils.start_workers)."""
        device = torch.device(device)
        files = TrainImageDataset(gt_dir, upscale).image_file_names
        if not files:
            raise ValueError(f"DeviceImageSet: no images under {gt_dir}")
        first = read_image_hwc(files[0])
        H, W, _ = first.shape
        _check_fits(len(files) * H * W * 3, device)
        store = torch.empty(len(files), H, W, 3, dtype=torch.uint8, device=device)
        chunk = max(1, min(len(files), _CHUNK_BYTES // (H * W * 3)))
        staging = torch.empty(chunk, H, W, 3, dtype=torch.uint8, pin_memory=device.type == "cuda")
        host = staging.numpy()

        def decode(j, i0):
            a = read_image_hwc(files[j])
            if a.shape != (H, W, 3):
                raise ValueError(f"DeviceImageSet: {files[j]} is {a.shape[1]}x{a.shape[0]}, the set's crops are {W}x{H} "
                                 f"(first file {files[0]}); every crop must have the same size")
            host[j - i0] = a

        with ThreadPoolExecutor(decode_threads()) as pool:
            for i0 in range(0, len(files), chunk):
                i1 = min(len(files), i0 + chunk)
                list(pool.map(decode, range(i0, i1), [i0] * (i1 - i0)))      # re-raises the first failure in file order
                store[i0:i1].copy_(staging[: i1 - i0])                        # synchronous: the staging buffer is reused next
        return cls(store, upscale)

    @classmethod
    def from_dataset(cls, ds, upscale: int, device) -> "DeviceImageSet":
        """Rebuild the uint8 store from the `gt` of a dataset whose items are (gt [3,H,W] fp32, lr).  Only sets on the 1/255 grid
        can: ValueError unless lut[round(gt * 255)] reproduces gt bit for bit."""
        device = torch.device(device)
        n = len(ds)
        if n == 0:
            raise ValueError("DeviceImageSet: empty dataset")
        table = lut("cpu")
        store = None
        for i in range(n):
            gt = ds[i][0]
            if not (isinstance(gt, Tensor) and gt.dim() == 3 and gt.shape[0] == 3):
                raise ValueError(f"DeviceImageSet: item {i}: gt must be a [3, H, W] tensor")
            gt = gt.detach().to("cpu", torch.float32)
            u = torch.round(gt * 255)
            if not bool(((u >= 0) & (u <= 255)).all()):
                raise ValueError(f"DeviceImageSet: item {i}: gt is outside [0, 1]")
            u8 = u.to(torch.uint8)
            if not torch.equal(table[u8.long()], gt):
                raise ValueError(f"DeviceImageSet: item {i}: gt is not on the 1/255 grid (lut[round(gt*255)] != gt); "
                                 "use the host loader (DATA.ON_DEVICE = False)")
            if store is None:
                H, W = gt.shape[1:]
                _check_fits(n * H * W * 3, device)
                store = torch.empty(n, H, W, 3, dtype=torch.uint8, device=device)
            elif tuple(gt.shape[1:]) != tuple(store.shape[1:3]):
                raise ValueError(f"DeviceImageSet: item {i} is {gt.shape[2]}x{gt.shape[1]}, the set's crops are "
                                 f"{store.shape[2]}x{store.shape[1]}")
            store[i].copy_(u8.permute(1, 2, 0))
        return cls(store, upscale)

    def batch(self, idx: Tensor, gt_out: Tensor | None = None, lr_out: Tensor | None = None, with_gt: bool = True,
              with_lr: bool = True):
        """ONE sst_gather_batch launch on the current stream: gt [B,3,H,W] = the crops idx names on the 1/255 grid, lr [B,3,oh,ow]
        = their x1/upscale bicubic.  idx: int32 [B] on the set's device (entries checked on the host by DeviceLoader).  Writes into
        gt_out / lr_out when given; with_gt / with_lr = False skips that output (returned as None)."""
        if idx.dtype != torch.int32 or idx.dim() != 1 or idx.device != self.device:
            raise ValueError(f"DeviceImageSet.batch: idx must be int32 [B] on {self.device}")
        B = idx.shape[0]
        gt = lr = None
        if with_gt:
            gt = gt_out if gt_out is not None else torch.empty(B, 3, self.H, self.W, device=self.device)
            _expect(gt, (B, 3, self.H, self.W), "gt_out")
        wy = iy = wx = ix = None
        Ty = Tx = 0
        if with_lr:
            lr = lr_out if lr_out is not None else torch.empty(B, 3, self.oh, self.ow, device=self.device)
            _expect(lr, (B, 3, self.oh, self.ow), "lr_out")
            wy, iy, wx, ix = self._bicubic.tables_i32(self.H, self.W, 1.0 / self.upscale, self.device)
            Ty, Tx = wy.shape[1], wx.shape[1]
        _abi.check(_abi.lib().sst_gather_batch(_abi.ptr(self.store), len(self), _abi.ptr(idx), B, self.H, self.W, _abi.ptr(self.lut),
                                               _abi.ptr(gt), _abi.ptr(lr), _abi.ptr(wy), _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix),
                                               self.oh, self.ow, Ty, Tx, _abi.stream_ptr()), "sst_gather_batch")
        return gt, lr


def _expect(t: Tensor, shape, name: str) -> None:
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"DeviceImageSet.batch: {name} must be contiguous fp32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


class DeviceTestSet:
    """The validation pairs on one device (config.DATA.VALIDATE_ON_DEVICE): decoded and copied ONCE, then iterated every epoch
    like DataLoader(ds, batch_size=1, shuffle=False) - (hr [1,3,H,W], lr [1,3,h,w]) fp32, bit-identical to what that loader
    yields.  Test images differ in size, so the store is a plain list of per-image tensors: no uniform-size store, no kernel."""

    def __init__(self, pairs):
        self.pairs = list(pairs)
        if not self.pairs:
            raise ValueError("DeviceTestSet: empty set")
        self.device = self.pairs[0][0].device

    def __len__(self) -> int:
        return len(self.pairs)

    def __iter__(self):
        # A DataLoader draws its base seed from the default CPU generator every time it is iterated, also with num_workers=0.
        # The same draw here: the training sampler's next shuffle, hence the training run, is then the same whichever way the
        # validation ran (tests/test_metrics_gpu.py compares the checkpoints of both).
        torch.empty((), dtype=torch.int64).random_()
        return iter(self.pairs)

    def __getitem__(self, i):
        return self.pairs[i]

    @classmethod
    def from_dataset(cls, ds, device) -> "DeviceTestSet":
        """From a dataset whose items are (hr [3,H,W], lr [3,h,w]) tensors, in the dataset's order.  Each image is sized against
        the free device memory before it is copied (MemoryError, as for the training set)."""
        device = torch.device(device)
        pairs = []
        for i in range(len(ds)):
            hr, lr = ds[i]
            for name, t in (("hr", hr), ("lr", lr)):
                if not (isinstance(t, Tensor) and t.dim() == 3):
                    raise ValueError(f"DeviceTestSet: item {i}: {name} must be a [C, H, W] tensor")
            # the default collate of a batch of one: stack = unsqueeze(0), values untouched
            hr, lr = hr.detach().unsqueeze(0).contiguous(), lr.detach().unsqueeze(0).contiguous()
            try:
                _check_fits(hr.numel() * hr.element_size() + lr.numel() * lr.element_size(), device)
            except MemoryError as e:
                raise MemoryError(f"DeviceTestSet: item {i} of {len(ds)} does not fit beside the training step ({e}); validate "
                                  "through the host loader (DATA.VALIDATE_ON_DEVICE = False)") from e
            pairs.append((hr.to(device), lr.to(device)))
        return cls(pairs)

    @classmethod
    def from_dir(cls, gt_dir: str, lr_dir: str, device) -> "DeviceTestSet":
        """TestImageDataset's file list and order."""
        return cls.from_dataset(TestImageDataset(gt_dir, lr_dir), device)


class DeviceLoader:
    """The training DataLoader's semantics (drop_last=True, shuffle through a sampler; DistributedSampler and its set_epoch work
    unchanged) over a DeviceImageSet.  Once per epoch the sampler's order becomes one int32 device tensor (one non-blocking
    host-to-device copy, index range checked on the host); step k is one gather launch on indices[k*B:(k+1)*B]."""

    def __init__(self, dset: DeviceImageSet, batch_size: int, sampler=None):
        if batch_size <= 0:
            raise ValueError("DeviceLoader: batch_size must be positive")
        self.dset = dset
        self.batch_size = int(batch_size)
        self.sampler = sampler if sampler is not None else torch.utils.data.RandomSampler(dset)
        self._gt = self._lr = None

    def __len__(self) -> int:
        return len(self.sampler) // self.batch_size

    def bind(self, gt: Tensor | None, lr: Tensor | None) -> None:
        """Later batches land in these buffers (the engine's static inputs: the step then copies nothing)."""
        self._gt, self._lr = gt, lr

    def plan(self) -> Tensor:
        """The epoch's index order on the host: int64 [len(self) * batch_size], every entry checked against the set's size."""
        order = torch.as_tensor(np.fromiter(iter(self.sampler), dtype=np.int64))
        order = order[: len(self) * self.batch_size]
        n = len(self.dset)
        if order.numel() and (int(order.min()) < 0 or int(order.max()) >= n):
            raise IndexError(f"DeviceLoader: the sampler produced an index outside [0, {n})")
        return order

    def __iter__(self):
        B = self.batch_size
        host = self.plan().to(torch.int32)
        dev = self.dset.device
        idx = host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host
        for k in range(len(self)):
            yield self.dset.batch(idx[k * B:(k + 1) * B], self._gt, self._lr)


def train_loader(config, train_dataset, world: int, rank: int):
    """The drivers' ON_DEVICE data path: (DeviceLoader, sampler or None).  The set comes from `train_dataset` when one is given
    (from_dataset), else from DATA.TRAIN_GT_IMAGES_DIR (from_dir); data-parallel ranks shard it with a DistributedSampler."""
    up = config.DATA.UPSCALE_FACTOR
    if train_dataset is not None:
        dset = DeviceImageSet.from_dataset(train_dataset, up, config.DEVICE)
    else:
        dset = DeviceImageSet.from_dir(config.DATA.TRAIN_GT_IMAGES_DIR, up, config.DEVICE)
    sampler = torch.utils.data.distributed.DistributedSampler(dset, world, rank, shuffle=True) if world > 1 else None
    return DeviceLoader(dset, config.DATA.BATCH_SIZE, sampler), sampler
