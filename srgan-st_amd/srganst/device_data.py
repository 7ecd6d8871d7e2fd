"""Training batches from an HBM-resident image set (config.DATA.ON_DEVICE).

The prepared HR crops are decoded ONCE and kept on the device as uint8 [N, H, W, 3] (HWC/RGB, as read_image decodes them); each
training batch is then ONE HIP launch (csrc/data.hip: sst_gather_batch) that gathers the batch's crops by index, converts them to
fp32 NCHW on the 1/255 grid and synthesises the x1/upscale bicubic LR in the same pass - the values TrainImageDataset + the
default collate produce (gt bit for bit; lr bit for bit with Bicubic("cuda")(gt), within the host-versus-device bound of the CPU
Bicubic).  No decode, no host-to-device copy and no sync per step.  The cost: the whole HR set in device memory on every rank.
With config.DATA.ON_DEVICE_WHOLE_IMAGES the device holds the WHOLE training images instead (DeviceImageArena: no crops cut
beforehand, images of any sizes) and the one launch per batch (sst_gather_crops) also cuts each sample's S x S window and applies one
of the eight dihedral transforms to it: DeviceCropLoader walks the tile grid data-prep/prepare_dataset.py would have written, or,
with DATA.RANDOM_CROP / DATA.AUGMENT, draws the window and the transform anew every epoch.
With DATA.DEGRADE that launch (sst_gather_crops_degraded) also blurs each sample with its own Gaussian kernel before the bicubic and
adds Gaussian noise after it (Degradation, the classical blind-SR model); degrade() is that stage alone on any fp32 batch.
With a JPEG quality in the sample's deg row (Degradation(jpeg_prob=...), DATA.DEGRADE_JPEG_PROB) a second launch (sst_jpeg) takes
the LR batch through an all-integer JPEG round trip in place; jpeg() is that stage alone.
With DATA.DEGRADE_SECOND (SecondOrder) the second-order stage of BSRGAN / Real-ESRGAN follows on the LR batch: a second blur with a
kernel from a table drawn per epoch (kernels.py: Gaussian, generalised Gaussian, plateau, sinc), gray / signal-dependent noise, a JPEG
pass and a final sinc filter before or after it - three sst_filter2d launches around one sst_jpeg; filter2d() is that stage alone.
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


def tile_grid(sizes, crop: int, step: int) -> np.ndarray:
    """The tiles data-prep/prepare_dataset.py:34-47 writes for images of these (H, W), as int32 [M, 3] rows (image, y0, x0): for
    each image, y0 in range(0, H - crop + 1, step), x0 in range(0, W - crop + 1, step), row-major.  An image smaller than
    `crop` on either side contributes nothing."""
    if crop <= 0 or step <= 0:
        raise ValueError(f"tile_grid: crop {crop} and step {step} must be positive")
    out = []
    for n, (h, w) in enumerate(sizes):
        ys, xs = np.arange(0, h - crop + 1, step), np.arange(0, w - crop + 1, step)     # empty when the image is too small
        if len(ys) and len(xs):
            g = np.empty((len(ys), len(xs), 3), np.int32)
            g[..., 0], g[..., 1], g[..., 2] = n, ys[:, None], xs[None, :]
            out.append(g.reshape(-1, 3))
    return np.concatenate(out) if out else np.empty((0, 3), np.int32)


def dihedral(c: Tensor, t: int) -> Tensor:
    """Transform t = 4*transpose + 2*vflip + 1*hflip of c [..., H, W], applied in that order (all eight dihedral elements):
    out[y][x] = c[sy][sx] with y' = t&2 ? S-1-y : y, x' = t&1 ? S-1-x : x and (sy, sx) = t&4 ? (x', y') : (y', x')."""
    if t & 4:
        c = c.transpose(-2, -1)
    if t & 2:
        c = c.flip(-2)
    if t & 1:
        c = c.flip(-1)
    return c


def crops_reference(images, desc, crop: int, upscale: int):
    """What one sst_gather_crops launch computes, in plain torch on the host: for each row (image, y0, x0, t) of desc the window
    images[image][y0:y0+crop, x0:x0+crop] (uint8 [H, W, 3]), transformed by dihedral(t), / 255 -> gt [B,3,crop,crop]; lr = the CPU
    Bicubic of gt (the data loader's host code).  The restatement the tests compare the kernel against."""
    desc = torch.as_tensor(np.asarray(desc)).reshape(-1, 4).tolist()
    gts = []
    for n, y0, x0, t in desc:
        im = torch.as_tensor(np.asarray(images[n]))
        if not (0 <= y0 and y0 + crop <= im.shape[0] and 0 <= x0 and x0 + crop <= im.shape[1] and 0 <= t < 8):
            raise ValueError(f"crops_reference: descriptor {(n, y0, x0, t)} is outside image {n} ({im.shape[0]}x{im.shape[1]})")
        c = im[y0:y0 + crop, x0:x0 + crop].permute(2, 0, 1)
        gts.append(dihedral(c, t).contiguous().float() / 255.0)
    gt = torch.stack(gts)
    return gt, Bicubic("cpu")(gt, scale=1.0 / upscale)


def _pad16(n: int) -> int:
    return (n + 15) & ~15


# ---- the blind-SR degradation stage (DATA.DEGRADE; csrc/degrade.h)
DEGRADE_TILE_COLS = 16           # LR columns of one workgroup of sst_degrade (csrc/degrade.h: deg::TILE_COLS; sst_degrade_tile_cols())
DEGRADE_KSIZES = tuple(range(3, 22, 2))
_DEGRADE_STREAM = 0x6A09E667F3BCC908      # keeps the loader's degradation generator apart from its window / transform generator


JPEG_CHROMA = {"444": 0, "420": 1}         # sst_jpeg's chroma argument
RESIZE_MODES = {"area": 0, "bilinear": 1, "bicubic": 2}       # the modes of sst_rescale and sst_rescale_to
# the first stage's random resize (DATA.DEGRADE_RESIZE; sst_rescale_to)
_RESIZE1_STREAM = 0x5BE0CD19137E2179      # keeps the loader's first-stage resize generator apart from its four others
RESIZE1_MAX_RATIO, RESIZE1_MIN_DIV, RESIZE1_MAX_DOWN = 2, 8, 16   # sst_rescale_to: H <= 8 hi, hi <= 2 H; h <= H <= 16 h


def resize1_size(n: int, s: float) -> int:
    """The intermediate length of an HR axis of n pixels at scale s: int(n s), at least ceil(n / 8)."""
    return max(int(n * s), -(-n // RESIZE1_MIN_DIV))


def rescale_to_size_ok(hi: int, wi: int, H: int, W: int) -> bool:
    """True when sst_rescale_to takes the intermediate size (hi, wi) on an [H, W] input: 0, 0 (keep), or both within
    [ceil(n / 8), 2 n] of their axis."""
    if hi == 0 and wi == 0:
        return True
    return (hi > 0 and wi > 0 and RESIZE1_MIN_DIV * hi >= H and hi <= RESIZE1_MAX_RATIO * H and RESIZE1_MIN_DIV * wi >= W
            and wi <= RESIZE1_MAX_RATIO * W)


def _chroma(mode, who: str) -> int:
    if mode not in JPEG_CHROMA:
        raise ValueError(f"{who}: jpeg_chroma must be '444' or '420', got {mode!r}")
    return JPEG_CHROMA[mode]


def degrade_rows(sigma1, sigma2, theta, noise255, keys, jpeg=None) -> np.ndarray:
    """The deg rows of the kernels, int32 [n, 8], from per-sample arrays: the Gaussian's standard deviations along its two axes
    (pixels; <= 0 in either: no blur, the row gets the sentinel qa = -1), the angle of the first axis against x = columns (radians; y
    = rows), the noise's standard deviation in 0..255 units and the Philox key [n, 2].  With [[A, B], [B, C]] the inverse of
    R(theta) diag(sigma1^2, sigma2^2) R(theta)^T the row holds (A/2, B, C/2), computed in fp64 and rounded once to fp32, then
    noise255 / 255, the key, the JPEG quality `jpeg` (per sample, 0..100; 0 or None: no JPEG stage) and a zero word."""
    s1, s2, th, nz = (np.atleast_1d(np.asarray(a, np.float64)) for a in (sigma1, sigma2, theta, noise255))
    n = len(s1)
    keys = np.asarray(keys, np.int64).reshape(n, 2) & 0xFFFFFFFF
    blur = (s1 > 0) & (s2 > 0)
    i1, i2 = 1.0 / np.where(blur, s1, 1.0) ** 2, 1.0 / np.where(blur, s2, 1.0) ** 2
    c, s = np.cos(th), np.sin(th)
    q = np.stack([0.5 * (c * c * i1 + s * s * i2), c * s * (i1 - i2), 0.5 * (s * s * i1 + c * c * i2), nz / 255.0], 1)
    q[~blur, :3] = (-1.0, 0.0, 0.0)
    rows = np.zeros((n, 8), np.int32)
    rows[:, :4] = q.astype(np.float32).view(np.int32)
    rows[:, 4:6] = keys.astype(np.uint32).view(np.int32)
    if jpeg is not None:
        rows[:, 6] = np.broadcast_to(np.asarray(jpeg, np.int64), (n,))
    return rows


class Degradation:
    """The per-sample parameters of the classical blind-SR degradation lr = quantise(clamp(bicubic_down(gt (*) k) + n)): k an
    anisotropic Gaussian on a ksize x ksize window, n Gaussian noise.  draw(n, generator) -> int32 [n, 8] on the host, one deg row
    per sample: sigma1, sigma2 uniform in blur_sigma (equal when aniso is off), theta uniform in [0, pi), the no-blur sentinel with
    probability 1 - blur_prob; the noise's standard deviation uniform in noise_sigma (0..255 units), 0 with probability
    1 - noise_prob; two random key words.  With jpeg_prob > 0 a sample also gets, with that probability, a JPEG quality that is a
    uniform integer in the closed range jpeg_quality (word 6 of its row; sst_jpeg, chroma mode jpeg_chroma): these draws are made
    after all the others, so the other words are the ones drawn without them.  Degradation.fixed(...) draws the same row every time
    (validation, tests).
    resize_prob = (up, down, keep), three probabilities that sum to 1 (Real-ESRGAN's first stage: (0.2, 0.7, 0.1); None: no resize,
    and every draw, repr and behaviour is the one of an instance built without these arguments): the stage becomes blur at the HR
    size (sst_blur), a resize to an intermediate size at a scale uniform in [1, resize_range[1]] (up) or [resize_range[0], 1]
    (down), the same on both axes, with a mode uniform in resize_modes, the noise THERE, and a resize to the LR size with a mode
    drawn independently (sst_rescale_to; no antialias).  draw() is unchanged; draw_resize(n, H, W, generator, deg_rows) -> int32
    [n, 8] makes the rows of the resize, with the deg rows' noise word and key in them."""

    def __init__(self, blur_sigma=(0.2, 4.0), aniso: bool = True, blur_prob: float = 1.0, noise_sigma=(0.0, 25.0),
                 noise_prob: float = 1.0, ksize: int = 21, jpeg_quality=(30, 95), jpeg_prob: float = 0.0, jpeg_chroma: str = "420",
                 resize_prob=None, resize_range=(0.15, 1.5), resize_modes=("area", "bilinear", "bicubic")):
        self.blur_sigma, self.noise_sigma = (float(blur_sigma[0]), float(blur_sigma[1])), (float(noise_sigma[0]), float(noise_sigma[1]))
        self.aniso, self.blur_prob, self.noise_prob, self.ksize = bool(aniso), float(blur_prob), float(noise_prob), int(ksize)
        self._fixed = None
        if not 0 < self.blur_sigma[0] <= self.blur_sigma[1]:
            raise ValueError(f"Degradation: blur_sigma {blur_sigma} must be 0 < lo <= hi")
        if not 0 <= self.noise_sigma[0] <= self.noise_sigma[1]:
            raise ValueError(f"Degradation: noise_sigma {noise_sigma} must be 0 <= lo <= hi")
        if not (0 <= self.blur_prob <= 1 and 0 <= self.noise_prob <= 1):
            raise ValueError(f"Degradation: blur_prob {blur_prob} and noise_prob {noise_prob} must be in [0, 1]")
        if self.ksize not in DEGRADE_KSIZES:
            raise ValueError(f"Degradation: ksize {ksize} must be odd and in 3..21")
        self.jpeg_quality, self.jpeg_prob, self.jpeg_chroma = (int(jpeg_quality[0]), int(jpeg_quality[1])), float(jpeg_prob), jpeg_chroma
        self._fixed_jpeg = 0
        if not (1 <= self.jpeg_quality[0] <= self.jpeg_quality[1] <= 100 and tuple(jpeg_quality) == self.jpeg_quality):
            raise ValueError(f"Degradation: jpeg_quality {jpeg_quality} must be integers 1 <= lo <= hi <= 100")
        if not 0 <= self.jpeg_prob <= 1:
            raise ValueError(f"Degradation: jpeg_prob {jpeg_prob} must be in [0, 1]")
        _chroma(jpeg_chroma, "Degradation")
        self.resize_prob = None if resize_prob is None else tuple(float(v) for v in resize_prob)
        if self.resize_prob is not None and (len(self.resize_prob) != 3 or min(self.resize_prob) < 0
                                             or abs(sum(self.resize_prob) - 1) > 1e-9):
            raise ValueError(f"Degradation: resize_prob {tuple(resize_prob)} must be three probabilities (up, down, keep) that sum to 1")
        self.resize_range = (float(resize_range[0]), float(resize_range[1]))
        if not 0 < self.resize_range[0] <= 1 <= self.resize_range[1] <= RESIZE1_MAX_RATIO:
            raise ValueError(f"Degradation: resize_range {tuple(resize_range)} must be 0 < lo <= 1 <= hi <= {RESIZE1_MAX_RATIO}")
        self.resize_modes = tuple(resize_modes)
        if not self.resize_modes or any(m not in RESIZE_MODES for m in self.resize_modes):
            raise ValueError(f"Degradation: resize_modes {tuple(resize_modes)} must be names of {tuple(RESIZE_MODES)}")
        self._fixed_resize = None

    @property
    def has_jpeg(self) -> bool:
        """True when a row this draws can hold a JPEG quality: the loader then issues the sst_jpeg launch after the gather."""
        return self._fixed_jpeg > 0 if self._fixed else self.jpeg_prob > 0

    @property
    def has_resize(self) -> bool:
        """True when the stage resizes at random on the way to LR: the loader then issues the plain gather, sst_blur and sst_rescale_to
        instead of the fused degraded gather."""
        return self._fixed_resize is not None if self._fixed else self.resize_prob is not None

    @classmethod
    def fixed(cls, sigma1: float, sigma2: float, theta_deg: float, noise: float, key=0, ksize: int = 21, jpeg: int = 0,
              jpeg_chroma: str = "420", resize=None) -> "Degradation":
        """Every sample gets these parameters: the two standard deviations (0: no blur), the angle in degrees, the noise's standard
        deviation in 0..255 units, the key (an int: the low and high 32 bits; or a pair of words), the JPEG quality (0: none) and the
        random resize's stand-in (None: none, the fused stage; (s, m1, m2): to the scale s in [0.125, 2] of the HR size with the mode
        m1, the noise there, to the LR size with m2)."""
        if resize is not None:
            if len(resize) != 3 or not 1 / RESIZE1_MIN_DIV <= float(resize[0]) <= RESIZE1_MAX_RATIO or resize[1] not in RESIZE_MODES \
                    or resize[2] not in RESIZE_MODES:
                raise ValueError(f"Degradation.fixed: resize {resize!r} must be (s, m1, m2), s in [{1 / RESIZE1_MIN_DIV}, "
                                 f"{RESIZE1_MAX_RATIO}], the modes of {tuple(RESIZE_MODES)}")
            resize = (float(resize[0]), resize[1], resize[2])
        if sigma1 < 0 or sigma2 < 0 or noise < 0 or (sigma1 > 0) != (sigma2 > 0):
            raise ValueError(f"Degradation.fixed: sigma ({sigma1}, {sigma2}) must be both positive or both 0, noise {noise} >= 0")
        if int(jpeg) != jpeg or not 0 <= jpeg <= 100:
            raise ValueError(f"Degradation.fixed: the JPEG quality {jpeg!r} must be an integer in 0..100 (0: none)")
        d = cls(ksize=ksize, jpeg_chroma=jpeg_chroma)
        d._fixed_jpeg = int(jpeg)
        k = (int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF) if isinstance(key, (int, np.integer)) else (int(key[0]), int(key[1]))
        d._fixed = (float(sigma1), float(sigma2), float(theta_deg), float(noise), k)
        d._fixed_resize = resize
        return d

    def __repr__(self) -> str:
        if self._fixed:
            s1, s2, th, nz, k = self._fixed
            jp = f", jpeg={self._fixed_jpeg}, jpeg_chroma={self.jpeg_chroma!r}" if self._fixed_jpeg else ""
            rs = f", resize={self._fixed_resize}" if self._fixed_resize else ""
            return f"Degradation.fixed(sigma1={s1:g}, sigma2={s2:g}, theta_deg={th:g}, noise={nz:g}, key={k}, ksize={self.ksize}{jp}{rs})"
        jp = f", jpeg_quality={self.jpeg_quality}, jpeg_prob={self.jpeg_prob:g}, jpeg_chroma={self.jpeg_chroma!r}" if self.jpeg_prob > 0 else ""
        rs = (f", resize_prob={self.resize_prob}, resize_range={self.resize_range}, resize_modes={self.resize_modes}"
              if self.resize_prob is not None else "")
        return (f"Degradation(blur_sigma={self.blur_sigma}, aniso={self.aniso}, blur_prob={self.blur_prob:g}, "
                f"noise_sigma={self.noise_sigma}, noise_prob={self.noise_prob:g}, ksize={self.ksize}{jp}{rs})")

    def draw(self, n: int, generator: torch.Generator | None = None) -> Tensor:
        if self._fixed:
            s1, s2, th, nz, k = self._fixed
            return torch.from_numpy(degrade_rows([s1] * n, [s2] * n, [np.deg2rad(th)] * n, [nz] * n, [k] * n, self._fixed_jpeg))
        u = torch.rand(n, 6, generator=generator, dtype=torch.float64).numpy()
        keys = torch.randint(0, 1 << 32, (n, 2), generator=generator, dtype=torch.int64).numpy()
        (b0, b1), (n0, n1) = self.blur_sigma, self.noise_sigma
        s1 = b0 + (b1 - b0) * u[:, 0]
        s2 = b0 + (b1 - b0) * u[:, 1] if self.aniso else s1
        blur = u[:, 3] < self.blur_prob
        nz = np.where(u[:, 5] < self.noise_prob, n0 + (n1 - n0) * u[:, 4], 0.0)
        jpeg = None
        if self.jpeg_prob > 0:                              # drawn last: every word above is the one drawn without the JPEG stage
            on = torch.rand(n, generator=generator, dtype=torch.float64).numpy() < self.jpeg_prob
            q = torch.randint(self.jpeg_quality[0], self.jpeg_quality[1] + 1, (n,), generator=generator, dtype=torch.int64).numpy()
            jpeg = np.where(on, q, 0)
        return torch.from_numpy(degrade_rows(np.where(blur, s1, 0.0), np.where(blur, s2, 0.0), np.pi * u[:, 2], nz, keys, jpeg))

    def draw_resize(self, n: int, H: int, W: int, generator: torch.Generator | None = None, deg_rows=None) -> Tensor:
        """The rows of the stage's random resize for n samples of an [H, W] HR batch, int32 [n, 8] (rescale_rows' layout, for
        rescale_to).  Per sample the kind (up, down, keep), then s uniform in [1, resize_range[1]] (up) or [resize_range[0], 1]
        (down), hi = max(int(H s), ceil(H / 8)) and wi likewise from the same s, then m1 and m2 uniform in resize_modes,
        independently; keep writes 0, 0 (the intermediate is the blurred HR image itself) and still draws m2, the mode of the resize
        to the LR size.  deg_rows: the stage's deg rows as draw() makes them - their sigma_n (word 3) and key (words 4, 5) go into
        the rows, shot and gray stay zero: the noise parameters of a sample are the ones drawn without resize."""
        if not self.has_resize:
            raise ValueError("Degradation.draw_resize: this stage has no resize (resize_prob is None)")
        rows = np.zeros((n, 8), np.int32)
        if self._fixed:
            s, m1, m2 = self._fixed_resize
            rows[:, 0], rows[:, 1], rows[:, 6] = resize1_size(H, s), resize1_size(W, s), RESIZE_MODES[m1] | RESIZE_MODES[m2] << 2
        else:
            u = torch.rand(n, 2, generator=generator, dtype=torch.float64).numpy()
            pick = torch.randint(0, 1 << 62, (n, 2), generator=generator, dtype=torch.int64).numpy()
            up, down, _ = self.resize_prob
            lo, hi = self.resize_range
            s = np.where(u[:, 0] < up, 1.0 + (hi - 1.0) * u[:, 1], lo + (1.0 - lo) * u[:, 1])
            keep = u[:, 0] >= up + down
            rows[:, 0] = np.where(keep, 0, [resize1_size(H, v) for v in s])
            rows[:, 1] = np.where(keep, 0, [resize1_size(W, v) for v in s])
            codes = np.array([RESIZE_MODES[m] for m in self.resize_modes], np.int32)
            rows[:, 6] = np.where(keep, 0, codes[pick[:, 0] % len(codes)]) | codes[pick[:, 1] % len(codes)] << 2
        if deg_rows is not None:
            a = np.asarray(deg_rows, np.int32).reshape(n, 8)
            rows[:, 2], rows[:, 4:6] = a[:, 3], a[:, 4:6]
        return torch.from_numpy(rows)

    @classmethod
    def from_config(cls, config) -> "Degradation | None":
        """DATA.DEGRADE_* -> a Degradation, or None with DATA.DEGRADE off."""
        data = config.DATA
        if not data.get("DEGRADE", False):
            return None
        return cls(data.DEGRADE_BLUR_SIGMA, data.DEGRADE_BLUR_ANISO, data.DEGRADE_BLUR_PROB, data.DEGRADE_NOISE_SIGMA,
                   data.DEGRADE_NOISE_PROB, data.DEGRADE_BLUR_KSIZE, tuple(data.get("DEGRADE_JPEG_QUALITY", (30, 95))),
                   data.get("DEGRADE_JPEG_PROB", 0.0), data.get("DEGRADE_JPEG_CHROMA", "420"),
                   tuple(data.get("DEGRADE_RESIZE_PROB", (0.2, 0.7, 0.1))) if data.get("DEGRADE_RESIZE", False) else None,
                   tuple(data.get("DEGRADE_RESIZE_RANGE", (0.15, 1.5))),
                   tuple(data.get("DEGRADE_RESIZE_MODES", ("area", "bilinear", "bicubic"))))


def _check_deg(deg: Tensor, B: int, device, who: str) -> None:
    if deg.dtype != torch.int32 or tuple(deg.shape) != (B, 8) or deg.device != device or not deg.is_contiguous():
        raise ValueError(f"{who}: deg must be contiguous int32 [{B}, 8] on {device}, got {deg.dtype} {tuple(deg.shape)} on {deg.device}")


_degrade_bicubic = {}


def jpeg(lr: Tensor, deg: Tensor, chroma: str = "420", out: Tensor | None = None) -> Tensor:
    """ONE sst_jpeg launch on the current stream: the JPEG stage alone on an fp32 batch lr [B,3,h,w] (h, w <= 8192) with the qualities
    in word 6 of the rows deg int32 [B,8] (0: the sample keeps its bits) -> a new tensor, or `out` (contiguous fp32 of lr's shape; out
    = lr runs in place).  An all-integer codec: the result is the same bits in every run and batch position."""
    c = _chroma(chroma, "jpeg")
    if lr.dtype != torch.float32 or lr.dim() != 4 or lr.shape[1] != 3 or not lr.is_cuda:
        raise ValueError(f"jpeg: lr must be fp32 [B, 3, h, w] on a ROCm device, got {lr.dtype} {tuple(lr.shape)} on {lr.device}")
    B, _, h, w = lr.shape
    _check_deg(deg, B, lr.device, "jpeg")
    if out is None:
        out = lr.clone(memory_format=torch.contiguous_format)
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(lr.shape) or not out.is_contiguous() or out.device != lr.device:
            raise ValueError(f"jpeg: out must be contiguous fp32 {tuple(lr.shape)} on {lr.device}, got {out.dtype} {tuple(out.shape)}")
        if out.data_ptr() != lr.data_ptr():
            out.copy_(lr)
    _abi.check(_abi.lib().sst_jpeg(_abi.ptr(out), _abi.ptr(deg), B, h, w, c, _abi.stream_ptr()), "sst_jpeg")
    return out


def blur(x: Tensor, deg: Tensor, ksize: int = 21, out: Tensor | None = None) -> Tensor:
    """ONE sst_blur launch on the current stream: the degradation stage's blur alone on an fp32 batch x [B,3,H,W] (ksize // 2 <
    min(H, W)) with the rows deg int32 [B,8] (Degradation.draw / degrade_rows; the noise word is not read) -> unquantised fp32
    [B,3,H,W], a new tensor, or `out` (contiguous fp32 of x's shape; never x itself).  A sample's result is the image sst_degrade
    makes before its bicubic, bit for bit; a row without blur keeps the sample's bits."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError(f"blur: x must be fp32 [B, 3, H, W] on a ROCm device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, _, H, W = x.shape
    _check_deg(deg, B, x.device, "blur")
    if out is None:
        out = torch.empty(B, 3, H, W, device=x.device)
    else:
        if out is x or out.data_ptr() == x.data_ptr():
            raise ValueError("blur: out must not be x (a tile reads its neighbours' pixels: out of place only)")
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"blur: out must be contiguous fp32 {tuple(x.shape)} on {x.device}, got {out.dtype} {tuple(out.shape)}")
    x = x.contiguous()
    _abi.check(_abi.lib().sst_blur(_abi.ptr(x), _abi.ptr(deg), _abi.ptr(out), B, H, W, int(ksize), _abi.stream_ptr()), "sst_blur")
    return out


def degrade(x: Tensor, deg: Tensor, scale: int, ksize: int = 21, quantise: bool = True, jpeg_chroma: str | None = None,
            resize_rows: Tensor | None = None) -> Tensor:
    """ONE sst_degrade launch on the current stream: the degradation stage on an fp32 batch x [B,3,H,W] of any size (H, W >= scale,
    ksize // 2 < min(H, W)) with per-sample rows deg int32 [B,8] (Degradation.draw / degrade_rows) -> lr [B,3,H//scale,W//scale].
    The stand-alone form of DeviceImageArena.crops(desc, deg=...), whose lr it reproduces from its gt bit for bit.  quantise=False
    (tests and tools) returns the unclamped, unrounded values.  jpeg_chroma ('444' / '420'): a second launch (sst_jpeg) takes lr
    through the JPEG stage in place, at the qualities in word 6 of the rows; it needs the quantised values.
    resize_rows: int32 [B,8] (Degradation.draw_resize) - the stage with its random resize, as the loader issues it: TWO launches
    instead of the one, blur(x, deg) and rescale_to(.., resize_rows, (H//scale, W//scale)), whose rows carry the noise."""
    if resize_rows is not None:
        if jpeg_chroma is not None:
            _chroma(jpeg_chroma, "degrade")
            if not quantise:
                raise ValueError("degrade: the JPEG stage works on the 1/255 grid; jpeg_chroma needs quantise=True")
        if scale not in (2, 4, 8):
            raise ValueError(f"degrade: scale must be 2, 4 or 8, got {scale!r}")
        lr = rescale_to(blur(x, deg, ksize), resize_rows, (int(x.shape[2] * (1.0 / scale)), int(x.shape[3] * (1.0 / scale))), quantise)
        if jpeg_chroma is not None:
            jpeg(lr, deg, jpeg_chroma, out=lr)
        return lr
    if jpeg_chroma is not None:
        _chroma(jpeg_chroma, "degrade")
        if not quantise:
            raise ValueError("degrade: the JPEG stage works on the 1/255 grid; jpeg_chroma needs quantise=True")
    if scale not in (2, 4, 8):
        raise ValueError(f"degrade: scale must be 2, 4 or 8, got {scale!r}")
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError(f"degrade: x must be fp32 [B, 3, H, W] on a ROCm device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, _, H, W = x.shape
    if H < scale or W < scale:
        raise ValueError(f"degrade: image {W}x{H} is smaller than the scale {scale}")
    _check_deg(deg, B, x.device, "degrade")
    bic = _degrade_bicubic.setdefault(x.device, Bicubic(str(x.device)))
    wy, iy, wx, ix = bic.tables_i32(H, W, 1.0 / scale, x.device)
    oh, ow = int(H * (1.0 / scale)), int(W * (1.0 / scale))
    x = x.contiguous()
    lr = torch.empty(B, 3, oh, ow, device=x.device)
    _abi.check(_abi.lib().sst_degrade(_abi.ptr(x), _abi.ptr(deg), B, H, W, int(ksize), int(bool(quantise)), _abi.ptr(lr), _abi.ptr(wy),
                                      _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), oh, ow, wy.shape[1], wx.shape[1],
                                      _abi.stream_ptr()), "sst_degrade")
    if jpeg_chroma is not None:
        jpeg(lr, deg, jpeg_chroma, out=lr)
    return lr


# ---- the second-order degradation stage (DATA.DEGRADE_SECOND; csrc/filter.hip)
_SECOND_STREAM = 0x3C6EF372FE94F82B       # keeps the loader's second-stage generator apart from its two others
_SECOND_BANK_STREAM = 0x510E527FADE682D1  # and the epoch's kernel bank apart from the per-tile rows
SECOND_FAMILIES = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")


def filter_rows(index, noise255, shot, gray, keys) -> np.ndarray:
    """The rows of sst_filter2d, int32 [n, 8], from per-sample arrays: the kernel's index in the bank (-1: no blur), the Gaussian
    noise's standard deviation in 0..255 units (stored / 255), the shot coefficient s_p itself (the noise's variance is
    sigma_n^2 + s_p * max(v, 0): a heteroscedastic Gaussian, not a Poisson sampler), the gray flag (one draw for the three channels)
    and the Philox key [n, 2].  Words 6 and 7 are zero."""
    idx = np.atleast_1d(np.asarray(index, np.int64))
    n = len(idx)
    nz, sp = (np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in (noise255, shot))
    gr = np.broadcast_to(np.asarray(gray), (n,))
    if not (np.isfinite(nz).all() and (nz >= 0).all() and np.isfinite(sp).all() and (sp >= 0).all()):
        raise ValueError("filter_rows: noise255 and shot must be finite and >= 0")
    if (idx < -1).any() or (idx > 0x7FFFFFFF).any():
        raise ValueError("filter_rows: a kernel index must be -1 (no blur) or an index into the bank")
    if not np.isin(gr, (0, 1)).all():
        raise ValueError("filter_rows: gray must be 0 or 1")
    keys = np.asarray(keys, np.int64).reshape(n, 2) & 0xFFFFFFFF
    rows = np.zeros((n, 8), np.int32)
    rows[:, 0] = idx
    rows[:, 1] = (nz / 255.0).astype(np.float32).view(np.int32)
    rows[:, 2] = sp.astype(np.float32).view(np.int32)
    rows[:, 3] = gr.astype(np.int32)
    rows[:, 4:6] = keys.astype(np.uint32).view(np.int32)
    return rows


def filter2d(x: Tensor, flt: Tensor, bank: Tensor | None, quantise: bool = True, out: Tensor | None = None) -> Tensor:
    """ONE sst_filter2d launch on the current stream: the second-order stage alone on an fp32 batch x [B,3,h,w] (h, w <= 8192) with
    the rows flt int32 [B,8] (filter_rows) and the kernel table bank fp32 [M,K,K] on x's device (kernels.bank; None: no kernels, noise
    only) -> a new tensor, or `out` (contiguous fp32 of x's shape; never x itself: a tile reads its neighbours' pixels).  Per sample:
    the correlation with its kernel under torch's `reflect` padding, noise, clamp to [0, 1] and the 1/255 grid; a row with neither a
    kernel nor noise keeps the sample's bits.  quantise=False (tests and tools) returns the unclamped, unrounded values."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError(f"filter2d: x must be fp32 [B, 3, h, w] on a ROCm device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, _, h, w = x.shape
    _check_deg(flt, B, x.device, "filter2d")
    M, K = 0, 3
    if bank is not None:
        if (bank.dtype != torch.float32 or bank.dim() != 3 or bank.shape[1] != bank.shape[2] or bank.device != x.device
                or not bank.is_contiguous()):
            raise ValueError(f"filter2d: bank must be contiguous fp32 [M, K, K] on {x.device}, got {bank.dtype} {tuple(bank.shape)} "
                             f"on {bank.device}")
        M, K = (bank.shape[0], bank.shape[1]) if bank.shape[0] else (0, 3)
    if out is None:
        out = torch.empty(B, 3, h, w, device=x.device)
    else:
        if out is x or out.data_ptr() == x.data_ptr():
            raise ValueError("filter2d: out must not be x (a tile reads its neighbours' pixels: out of place only)")
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"filter2d: out must be contiguous fp32 {tuple(x.shape)} on {x.device}, got {out.dtype} {tuple(out.shape)}")
    x = x.contiguous()
    _abi.check(_abi.lib().sst_filter2d(_abi.ptr(x), _abi.ptr(out), _abi.ptr(flt), _abi.ptr(bank) if M else None, M, B, h, w, K,
                                       int(bool(quantise)), _abi.stream_ptr()), "sst_filter2d")
    return out


# ---- the random resize round trip inside the second stage (DATA.DEGRADE2_RESIZE; csrc/resize.hip)
_RESIZE_STREAM = 0x1F83D9ABFB41BD6B       # keeps the loader's resize generator apart from its three others
RESIZE_MAX_RATIO, RESIZE_MIN_DIV = 2, 4   # sst_rescale's limits on an intermediate size: h <= 4 hi and hi <= 2 h


def resize_size(n: int, s: float) -> int:
    """The intermediate length of an axis of n pixels at scale s: int(n s), at least ceil(n / 4)."""
    return max(int(n * s), -(-n // RESIZE_MIN_DIV))


def rescale_size_ok(hi: int, wi: int, h: int, w: int) -> bool:
    """True when sst_rescale takes the intermediate size (hi, wi) on an [h, w] image: 0, 0 (no resize), or both within
    [ceil(n / 4), 2 n] of their axis."""
    if hi == 0 and wi == 0:
        return True
    return (hi > 0 and wi > 0 and RESIZE_MIN_DIV * hi >= h and hi <= RESIZE_MAX_RATIO * h and RESIZE_MIN_DIV * wi >= w
            and wi <= RESIZE_MAX_RATIO * w)


def rescale_rows(size, modes, noise255, shot, gray, keys) -> np.ndarray:
    """The rows of sst_rescale, int32 [n, 8], n = the number of keys [n, 2]: per sample the intermediate size (`size`: None or 0 for
    no resize in any sample, else per sample None, 0 or (hi, wi)), the pair of mode names (`modes`: one pair for all, or a pair per
    sample; "area" | "bilinear" | "bicubic"; the first for the resize to (hi, wi), the second for the resize back), then filter_rows'
    noise arguments: the Gaussian noise's standard deviation in 0..255 units (stored / 255), the shot coefficient, the gray flag and
    the Philox key.  Word 6 is m1 | m2 << 2 | gray << 4, word 7 zero."""
    keys = np.asarray(keys, np.int64).reshape(-1, 2) & 0xFFFFFFFF
    n = len(keys)
    nz, sp = (np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in (noise255, shot))
    gr = np.broadcast_to(np.asarray(gray), (n,))
    if not (np.isfinite(nz).all() and (nz >= 0).all() and np.isfinite(sp).all() and (sp >= 0).all()):
        raise ValueError("rescale_rows: noise255 and shot must be finite and >= 0")
    if not np.isin(gr, (0, 1)).all():
        raise ValueError("rescale_rows: gray must be 0 or 1")
    sizes = np.zeros((n, 2), np.int64)
    none = lambda s: s is None or (isinstance(s, (int, np.integer)) and s == 0)
    if not none(size):
        if len(size) != n:
            raise ValueError(f"rescale_rows: {len(size)} sizes for {n} keys")
        for i, s in enumerate(size):
            if none(s):
                continue
            if np.ndim(s) != 1 or len(s) != 2 or any(int(v) != v for v in s):
                raise ValueError(f"rescale_rows: a size must be None, 0 or a pair of integers (hi, wi), got {s!r}")
            sizes[i] = (int(s[0]), int(s[1]))
    if (sizes < 0).any() or (sizes > 0x7FFFFFFF).any() or ((sizes[:, 0] == 0) != (sizes[:, 1] == 0)).any():
        raise ValueError("rescale_rows: an intermediate size must be two positive integers, or 0, 0 (no resize)")
    modes = [modes] * n if len(modes) == 2 and all(isinstance(m, str) for m in modes) else list(modes)
    if len(modes) != n:
        raise ValueError(f"rescale_rows: {len(modes)} mode pairs for {n} keys")
    for pair in modes:
        if len(pair) != 2 or pair[0] not in RESIZE_MODES or pair[1] not in RESIZE_MODES:
            raise ValueError(f"rescale_rows: modes must be pairs of {tuple(RESIZE_MODES)}, got {pair!r}")
    rows = np.zeros((n, 8), np.int32)
    rows[:, 0:2] = sizes
    rows[:, 2] = (nz / 255.0).astype(np.float32).view(np.int32)
    rows[:, 3] = sp.astype(np.float32).view(np.int32)
    rows[:, 4:6] = keys.astype(np.uint32).view(np.int32)
    rows[:, 6] = [RESIZE_MODES[a] | RESIZE_MODES[b] << 2 for a, b in modes]
    rows[:, 6] |= gr.astype(np.int32) << 4
    return rows


def rescale(x: Tensor, rows: Tensor, quantise: bool = True, out: Tensor | None = None) -> Tensor:
    """ONE sst_rescale launch on the current stream: the resize round trip alone on an fp32 batch x [B,3,h,w] (h, w <= 8192) with the
    rows int32 [B,8] (rescale_rows) -> a new tensor, or `out` (contiguous fp32 of x's shape; never x itself).  Per sample: resample
    to its intermediate size with its first mode, noise there, resample back to (h, w) with its second mode, clamp to [0, 1] and the
    1/255 grid; a row with neither a size nor noise keeps the sample's bits.  quantise=False (tests and tools) returns the unclamped,
    unrounded values.  rows on x's device are taken as they are (a size outside the kernel's limits makes that sample NaN); rows on
    the host are checked first - a size outside [ceil(n / 4), 2 n] of its axis raises - and then uploaded."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError(f"rescale: x must be fp32 [B, 3, h, w] on a ROCm device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, _, h, w = x.shape
    if rows.device.type == "cpu" and rows.dtype == torch.int32 and tuple(rows.shape) == (B, 8):
        for b, (hi, wi) in enumerate(rows[:, :2].tolist()):
            if not rescale_size_ok(hi, wi, h, w):
                raise ValueError(f"rescale: row {b}: the intermediate size {hi}x{wi} (rows x columns) must be 0, 0 or within "
                                 f"[ceil(n / {RESIZE_MIN_DIV}), {RESIZE_MAX_RATIO} n] of each axis of the {h}x{w} image")
        rows = rows.contiguous().to(x.device)
    _check_deg(rows, B, x.device, "rescale")
    if out is None:
        out = torch.empty(B, 3, h, w, device=x.device)
    else:
        if out is x or out.data_ptr() == x.data_ptr():
            raise ValueError("rescale: out must not be x (a tile reads its neighbours' pixels: out of place only)")
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"rescale: out must be contiguous fp32 {tuple(x.shape)} on {x.device}, got {out.dtype} {tuple(out.shape)}")
    x = x.contiguous()
    _abi.check(_abi.lib().sst_rescale(_abi.ptr(x), _abi.ptr(out), _abi.ptr(rows), B, h, w, int(bool(quantise)), _abi.stream_ptr()),
               "sst_rescale")
    return out


def rescale_to(x: Tensor, rows: Tensor, size, quantise: bool = True, out: Tensor | None = None) -> Tensor:
    """ONE sst_rescale_to launch on the current stream: rescale's chain with an output size of its own, on an fp32 batch x [B,3,H,W]
    (H, W <= 8192) with the rows int32 [B,8] (rescale_rows) -> [B,3,h,w], size = (h, w) with h <= H <= 16 h and w <= W <= 16 w: a
    new tensor, or `out` (contiguous fp32 of that shape; never x itself).  Per sample: resample to its intermediate size with its
    first mode (0, 0: the intermediate is x itself), noise there, resample to (h, w) with its second mode, clamp to [0, 1] and the
    1/255 grid; at (h, w) = (H, W) the bits are rescale's.  quantise=False (tests and tools) returns the unclamped, unrounded values.
    rows on x's device are taken as they are (a size outside the kernel's limits makes that sample NaN); rows on the host are
    checked first - a size outside [ceil(n / 8), 2 n] of its axis raises - and then uploaded."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError(f"rescale_to: x must be fp32 [B, 3, H, W] on a ROCm device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, _, H, W = x.shape
    if np.ndim(size) != 1 or len(size) != 2 or any(int(v) != v for v in size):
        raise ValueError(f"rescale_to: size must be a pair of integers (h, w), got {size!r}")
    h, w = int(size[0]), int(size[1])
    if not (1 <= h <= H <= RESIZE1_MAX_DOWN * h and 1 <= w <= W <= RESIZE1_MAX_DOWN * w):
        raise ValueError(f"rescale_to: the output size {h}x{w} (rows x columns) must be within [n / {RESIZE1_MAX_DOWN}, n] of each axis "
                         f"of the {H}x{W} input")
    if rows.device.type == "cpu" and rows.dtype == torch.int32 and tuple(rows.shape) == (B, 8):
        for b, (hi, wi) in enumerate(rows[:, :2].tolist()):
            if not rescale_to_size_ok(hi, wi, H, W):
                raise ValueError(f"rescale_to: row {b}: the intermediate size {hi}x{wi} (rows x columns) must be 0, 0 or within "
                                 f"[ceil(n / {RESIZE1_MIN_DIV}), {RESIZE1_MAX_RATIO} n] of each axis of the {H}x{W} image")
        rows = rows.contiguous().to(x.device)
    _check_deg(rows, B, x.device, "rescale_to")
    if out is None:
        out = torch.empty(B, 3, h, w, device=x.device)
    else:
        if out is x or out.data_ptr() == x.data_ptr():
            raise ValueError("rescale_to: out must not be x (a tile reads its neighbours' pixels: out of place only)")
        if out.dtype != torch.float32 or tuple(out.shape) != (B, 3, h, w) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"rescale_to: out must be contiguous fp32 {(B, 3, h, w)} on {x.device}, got {out.dtype} {tuple(out.shape)}")
    x = x.contiguous()
    _abi.check(_abi.lib().sst_rescale_to(_abi.ptr(x), _abi.ptr(out), _abi.ptr(rows), B, H, W, h, w, int(bool(quantise)),
                                         _abi.stream_ptr()), "sst_rescale_to")
    return out


def _range(v, name: str, lo_min: float = 0.0, strict: bool = False):
    a, b = float(v[0]), float(v[1])
    if not ((lo_min < a if strict else lo_min <= a) and a <= b and np.isfinite(b)):
        raise ValueError(f"SecondOrder: {name} {tuple(v)} must be {lo_min:g} {'<' if strict else '<='} lo <= hi")
    return a, b


class SecondOrder:
    """The parameters of the second degradation stage (BSRGAN / Real-ESRGAN's second order), applied to the first stage's LR batch:
      A  blur 2 with a kernel of the epoch's bank (probability blur_prob) and noise 2 (noise_prob): Gaussian with a standard deviation
         uniform in noise_sigma (0..255 units), or with probability shot_prob signal-dependent, s_p with sqrt(s_p) uniform between the
         roots of `shot`; gray (one draw for the three channels) with probability gray_prob
      B  the final sinc filter (final_sinc_prob, cutoff uniform in omega) for the samples that take it BEFORE the JPEG pass
         (sinc_first_prob), the others passed through
      J  JPEG at a quality that is a uniform integer in jpeg_quality (jpeg_prob)
      C  the final sinc filter for the other samples.
    draw_bank(generator) -> fp32 [bank_size + sinc_bank_size, ksize, ksize] on the host: bank_size blur kernels, each a sinc
    (sinc_prob) or of one of the six families of family_prob (iso / aniso Gaussian, generalised Gaussian, plateau) with standard
    deviations uniform in blur_sigma at a uniform angle, on a window `support` that is odd and uniform in 7..ksize; then
    sinc_bank_size final-sinc kernels.  draw(n, generator) -> int32 [4, n, 8] on the host: the rows of A, B, J (word 6: the quality,
    as sst_jpeg reads it) and C.  SecondOrder.fixed(...) draws the same bank and rows every time (validation, tests).
    resize_prob = (up, down, keep), three probabilities that sum to 1 (Real-ESRGAN's second stage: (0.3, 0.4, 0.3); None: no resize,
    and every draw is the one made without these arguments): between A's blur and B the sample makes a resize round trip R
    (sst_rescale) - to an intermediate size at a scale uniform in [1, resize_range[1]] (up) or [resize_range[0], 1] (down), the same
    on both axes, with a mode uniform in resize_modes, then noise 2 THERE, then back to the LR size with a mode drawn independently.
    draw() then leaves A's noise words zero (keep_noise=True: as drawn), and draw_resize(n, h, w, generator, noise=A's rows as drawn)
    -> int32 [n, 8] makes the rows of R with that noise in them: the noise parameters of a sample are the ones drawn without resize."""

    def __init__(self, blur_prob: float = 0.8, blur_sigma=(0.2, 1.5), family_prob=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03),
                 beta_gaussian=(0.5, 4.0), beta_plateau=(1.0, 2.0), sinc_prob: float = 0.1, noise_prob: float = 1.0,
                 noise_sigma=(1.0, 25.0), shot=(1e-5, 0.025), shot_prob: float = 0.5, gray_prob: float = 0.4,
                 final_sinc_prob: float = 0.8, omega=(np.pi / 3, np.pi), sinc_first_prob: float = 0.5, jpeg_quality=(30, 95),
                 jpeg_prob: float = 1.0, ksize: int = 21, bank_size: int = 1024, sinc_bank_size: int = 256, jpeg_chroma: str = "420",
                 resize_prob=None, resize_range=(0.3, 1.2), resize_modes=("area", "bilinear", "bicubic")):
        self.blur_sigma = _range(blur_sigma, "blur_sigma", strict=True)
        self.beta_gaussian = _range(beta_gaussian, "beta_gaussian", strict=True)
        self.beta_plateau = _range(beta_plateau, "beta_plateau", strict=True)
        self.noise_sigma, self.shot = _range(noise_sigma, "noise_sigma"), _range(shot, "shot")
        self.omega = _range(omega, "omega", strict=True)
        if self.omega[1] > np.pi:
            raise ValueError(f"SecondOrder: omega {tuple(omega)} must be within (0, pi]")
        probs = dict(blur_prob=blur_prob, sinc_prob=sinc_prob, noise_prob=noise_prob, shot_prob=shot_prob, gray_prob=gray_prob,
                     final_sinc_prob=final_sinc_prob, sinc_first_prob=sinc_first_prob, jpeg_prob=jpeg_prob)
        for name, v in probs.items():
            if not 0 <= v <= 1:
                raise ValueError(f"SecondOrder: {name} {v!r} must be in [0, 1]")
            setattr(self, name, float(v))
        self.family_prob = tuple(float(v) for v in family_prob)
        if len(self.family_prob) != 6 or min(self.family_prob) < 0 or abs(sum(self.family_prob) - 1) > 1e-9:
            raise ValueError(f"SecondOrder: family_prob {tuple(family_prob)} must be six probabilities that sum to 1 {SECOND_FAMILIES}")
        self.jpeg_quality, self.jpeg_chroma = (int(jpeg_quality[0]), int(jpeg_quality[1])), jpeg_chroma
        if not (1 <= self.jpeg_quality[0] <= self.jpeg_quality[1] <= 100 and tuple(jpeg_quality) == self.jpeg_quality):
            raise ValueError(f"SecondOrder: jpeg_quality {jpeg_quality} must be integers 1 <= lo <= hi <= 100")
        _chroma(jpeg_chroma, "SecondOrder")
        self.ksize, self.bank_size, self.sinc_bank_size = int(ksize), int(bank_size), int(sinc_bank_size)
        if self.ksize not in DEGRADE_KSIZES:
            raise ValueError(f"SecondOrder: ksize {ksize} must be odd and in 3..21")
        if self.bank_size < 1 or self.sinc_bank_size < 1:
            raise ValueError(f"SecondOrder: bank_size {bank_size} and sinc_bank_size {sinc_bank_size} must be positive")
        self.resize_prob = None if resize_prob is None else tuple(float(v) for v in resize_prob)
        if self.resize_prob is not None and (len(self.resize_prob) != 3 or min(self.resize_prob) < 0
                                             or abs(sum(self.resize_prob) - 1) > 1e-9):
            raise ValueError(f"SecondOrder: resize_prob {tuple(resize_prob)} must be three probabilities (up, down, keep) that sum to 1")
        self.resize_range = (float(resize_range[0]), float(resize_range[1]))
        if not 0 < self.resize_range[0] <= 1 <= self.resize_range[1] <= RESIZE_MAX_RATIO:
            raise ValueError(f"SecondOrder: resize_range {tuple(resize_range)} must be 0 < lo <= 1 <= hi <= {RESIZE_MAX_RATIO}")
        self.resize_modes = tuple(resize_modes)
        if not self.resize_modes or any(m not in RESIZE_MODES for m in self.resize_modes):
            raise ValueError(f"SecondOrder: resize_modes {tuple(resize_modes)} must be names of {tuple(RESIZE_MODES)}")
        self._fixed = None

    @property
    def has_jpeg(self) -> bool:
        """True when a row this draws can hold a JPEG quality: the loader then issues the stage's sst_jpeg launch."""
        return self._fixed["jpeg"] > 0 if self._fixed else self.jpeg_prob > 0

    @property
    def has_resize(self) -> bool:
        """True when the stage has the resize round trip R: the loader then issues the sst_rescale launch after A."""
        return self._fixed.get("resize") is not None if self._fixed else self.resize_prob is not None

    @classmethod
    def fixed(cls, kernel=None, noise: float = 0.0, shot: float = 0.0, gray: bool = False, key=0, sinc_omega: float | None = None,
              sinc_first: bool = True, jpeg: int = 0, ksize: int = 21, jpeg_chroma: str = "420", resize=None) -> "SecondOrder":
        """Every sample gets these: the blur kernel (a [ksize, ksize] table; None: no blur), the noise's standard deviation in 0..255
        units and shot coefficient, the gray flag, the key (an int: the low and high 32 bits; or a pair of words), the final sinc
        filter's cutoff (None: none) before (sinc_first) or after the JPEG pass, the JPEG quality (0: none), and the resize round
        trip (None: none; (s, m1, m2): to the scale s in [0.25, 2] with the mode m1, the noise there, back with m2)."""
        from . import kernels
        if int(jpeg) != jpeg or not 0 <= jpeg <= 100:
            raise ValueError(f"SecondOrder.fixed: the JPEG quality {jpeg!r} must be an integer in 0..100 (0: none)")
        if resize is not None:
            if len(resize) != 3 or not 1 / RESIZE_MIN_DIV <= float(resize[0]) <= RESIZE_MAX_RATIO or resize[1] not in RESIZE_MODES \
                    or resize[2] not in RESIZE_MODES:
                raise ValueError(f"SecondOrder.fixed: resize {resize!r} must be (s, m1, m2), s in [{1 / RESIZE_MIN_DIV}, "
                                 f"{RESIZE_MAX_RATIO}], the modes of {tuple(RESIZE_MODES)}")
            resize = (float(resize[0]), resize[1], resize[2])
        d = cls(ksize=ksize, jpeg_chroma=jpeg_chroma)
        tables = []
        if kernel is not None:
            kernel = np.asarray(kernel, np.float64)
            if kernel.shape != (d.ksize, d.ksize):
                raise ValueError(f"SecondOrder.fixed: the kernel must be a [{d.ksize}, {d.ksize}] table, got {kernel.shape}")
            tables.append(kernel)
        if sinc_omega is not None:
            tables.append(kernels.sinc(d.ksize, float(sinc_omega)))
        k = (int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF) if isinstance(key, (int, np.integer)) else (int(key[0]), int(key[1]))
        filter_rows([-1], noise, shot, int(bool(gray)), [k])                         # the refusals
        d._fixed = dict(bank=kernels.bank(tables) if tables else np.zeros((0, d.ksize, d.ksize), np.float32),
                        blur=0 if kernel is not None else -1, sinc=-1 if sinc_omega is None else len(tables) - 1,
                        noise=float(noise), shot=float(shot), gray=int(bool(gray)), key=k, sinc_first=bool(sinc_first), jpeg=int(jpeg),
                        omega=sinc_omega, resize=resize)
        return d

    def __repr__(self) -> str:
        if self._fixed:
            f = self._fixed
            return (f"SecondOrder.fixed(kernel={'a table' if f['blur'] >= 0 else None}, noise={f['noise']:g}, shot={f['shot']:g}, "
                    f"gray={bool(f['gray'])}, key={f['key']}, sinc_omega={f['omega']}, sinc_first={f['sinc_first']}, jpeg={f['jpeg']}, "
                    f"ksize={self.ksize}" + (f", resize={f['resize']}" if f.get("resize") else "") + ")")
        rs = (f", resize_prob={self.resize_prob}, resize_range={self.resize_range}, resize_modes={self.resize_modes}"
              if self.resize_prob is not None else "")
        return (f"SecondOrder(blur_prob={self.blur_prob:g}, blur_sigma={self.blur_sigma}, family_prob={self.family_prob}, "
                f"beta_gaussian={self.beta_gaussian}, beta_plateau={self.beta_plateau}, sinc_prob={self.sinc_prob:g}, "
                f"noise_prob={self.noise_prob:g}, noise_sigma={self.noise_sigma}, shot={self.shot}, shot_prob={self.shot_prob:g}, "
                f"gray_prob={self.gray_prob:g}, final_sinc_prob={self.final_sinc_prob:g}, omega=({self.omega[0]:.4g}, {self.omega[1]:.4g}), "
                f"sinc_first_prob={self.sinc_first_prob:g}, jpeg_quality={self.jpeg_quality}, jpeg_prob={self.jpeg_prob:g}, "
                f"jpeg_chroma={self.jpeg_chroma!r}, ksize={self.ksize}, bank_size={self.bank_size}+{self.sinc_bank_size}{rs})")

    def _support(self, u: float) -> int:
        lo = min(7, self.ksize)
        return lo + 2 * min(int(u * ((self.ksize - lo) // 2 + 1)), (self.ksize - lo) // 2)

    def draw_bank(self, generator: torch.Generator | None = None) -> np.ndarray:
        from . import kernels
        if self._fixed:
            return self._fixed["bank"]
        K, n = self.ksize, self.bank_size
        u = torch.rand(n + self.sinc_bank_size, 8, generator=generator, dtype=torch.float64).numpy()
        edges = np.cumsum(self.family_prob)
        (b0, b1), (w0, w1) = self.blur_sigma, self.omega
        tables = []
        for m in range(n):
            support = self._support(u[m, 1])
            if u[m, 0] < self.sinc_prob:
                tables.append(kernels.sinc(K, w0 + (w1 - w0) * u[m, 2], support))
                continue
            fam = min(int(np.searchsorted(edges, u[m, 3], side="right")), 5)
            s1 = b0 + (b1 - b0) * u[m, 4]
            s2 = b0 + (b1 - b0) * u[m, 5] if fam % 2 else s1
            theta = np.pi * u[m, 6] if fam % 2 else 0.0
            if fam < 2:
                tables.append(kernels.gaussian(K, s1, s2, theta, support))
            elif fam < 4:
                g0, g1 = self.beta_gaussian
                tables.append(kernels.generalized_gaussian(K, s1, s2, theta, g0 + (g1 - g0) * u[m, 7], support))
            else:
                p0, p1 = self.beta_plateau
                tables.append(kernels.plateau(K, s1, s2, theta, p0 + (p1 - p0) * u[m, 7], support))
        for m in range(n, n + self.sinc_bank_size):
            tables.append(kernels.sinc(K, w0 + (w1 - w0) * u[m, 2], self._support(u[m, 1])))
        return kernels.bank(tables)

    def draw_resize(self, n: int, h: int, w: int, generator: torch.Generator | None = None, noise=None) -> Tensor:
        """The rows of R for n samples of an [h, w] LR batch, int32 [n, 8] (rescale_rows' layout).  Per sample the kind (up, down,
        keep), then s uniform in [1, resize_range[1]] (up) or [resize_range[0], 1] (down), hi = max(int(h s), ceil(h / 4)) and wi
        likewise from the same s, then m1 and m2 uniform in resize_modes, independently; keep writes 0, 0.  noise: A's rows as drawn
        (draw(..., keep_noise=True)[0], filter_rows' layout) - their sigma, shot coefficient, gray flag and key go into the rows; a
        sample that keeps its size, has no noise but a blur in A then gets the size (h, w), the exact identity, so that R still puts
        it on the 1/255 grid, which A (launched unquantised beside R) no longer does."""
        if not self.has_resize:
            raise ValueError("SecondOrder.draw_resize: this stage has no resize (resize_prob is None)")
        rows = np.zeros((n, 8), np.int32)
        if self._fixed:
            s, m1, m2 = self._fixed["resize"]
            rows[:, 0], rows[:, 1], rows[:, 6] = resize_size(h, s), resize_size(w, s), RESIZE_MODES[m1] | RESIZE_MODES[m2] << 2
        else:
            u = torch.rand(n, 2, generator=generator, dtype=torch.float64).numpy()
            pick = torch.randint(0, 1 << 62, (n, 2), generator=generator, dtype=torch.int64).numpy()
            up, down, _ = self.resize_prob
            lo, hi = self.resize_range
            s = np.where(u[:, 0] < up, 1.0 + (hi - 1.0) * u[:, 1], lo + (1.0 - lo) * u[:, 1])
            keep = u[:, 0] >= up + down
            rows[:, 0] = np.where(keep, 0, [resize_size(h, v) for v in s])
            rows[:, 1] = np.where(keep, 0, [resize_size(w, v) for v in s])
            codes = np.array([RESIZE_MODES[m] for m in self.resize_modes], np.int32)
            rows[:, 6] = np.where(keep, 0, codes[pick[:, 0] % len(codes)] | codes[pick[:, 1] % len(codes)] << 2)
        if noise is not None:
            a = np.asarray(noise, np.int32).reshape(n, 8)
            rows[:, 2:4], rows[:, 4:6] = a[:, 1:3], a[:, 4:6]
            rows[:, 6] |= (a[:, 3] & 1) << 4
            bare = (rows[:, 0] == 0) & (a[:, 0] >= 0) & (a[:, 1] == 0) & (a[:, 2] == 0)
            rows[bare, 0], rows[bare, 1] = h, w
        return torch.from_numpy(rows)

    def draw(self, n: int, generator: torch.Generator | None = None, keep_noise: bool = False) -> Tensor:
        rows = self._draw(n, generator)
        if self.has_resize and not keep_noise:
            rows[0, :, 1:4] = 0                              # sigma, shot and gray: R adds this noise at its intermediate size
        return torch.from_numpy(rows)

    def _draw(self, n: int, generator) -> np.ndarray:
        rows = np.zeros((4, n, 8), np.int32)
        if self._fixed:
            f = self._fixed
            rows[0] = filter_rows([f["blur"]] * n, f["noise"], f["shot"], f["gray"], [f["key"]] * n)
            first = f["sinc"] >= 0 and f["sinc_first"]
            rows[1, :, 0] = f["sinc"] if first else -1
            rows[2, :, 6] = f["jpeg"]
            rows[3, :, 0] = -1 if first else f["sinc"]
            return rows
        u = torch.rand(n, 8, generator=generator, dtype=torch.float64).numpy()
        keys = torch.randint(0, 1 << 32, (n, 2), generator=generator, dtype=torch.int64).numpy()
        pick = torch.randint(0, 1 << 62, (n, 3), generator=generator, dtype=torch.int64).numpy()
        blur = np.where(u[:, 0] < self.blur_prob, pick[:, 0] % self.bank_size, -1)
        noisy, shot = u[:, 1] < self.noise_prob, u[:, 2] < self.shot_prob
        (n0, n1), (s0, s1) = self.noise_sigma, (np.sqrt(self.shot[0]), np.sqrt(self.shot[1]))
        nz = np.where(noisy & ~shot, n0 + (n1 - n0) * u[:, 3], 0.0)
        sp = np.where(noisy & shot, np.clip((s0 + (s1 - s0) * u[:, 3]) ** 2, *self.shot), 0.0)
        rows[0] = filter_rows(blur, nz, sp, (u[:, 4] < self.gray_prob).astype(np.int32), keys)
        sinc = np.where(u[:, 5] < self.final_sinc_prob, self.bank_size + pick[:, 1] % self.sinc_bank_size, -1)
        first = u[:, 6] < self.sinc_first_prob
        rows[1, :, 0] = np.where(first, sinc, -1)
        q0, q1 = self.jpeg_quality
        rows[2, :, 6] = np.where(u[:, 7] < self.jpeg_prob, q0 + pick[:, 2] % (q1 - q0 + 1), 0)
        rows[3, :, 0] = np.where(first, -1, sinc)
        return rows

    @classmethod
    def from_config(cls, config) -> "SecondOrder | None":
        """DATA.DEGRADE2_* -> a SecondOrder, or None with DATA.DEGRADE_SECOND off."""
        d = config.DATA
        if not d.get("DEGRADE_SECOND", False):
            return None
        return cls(d.DEGRADE2_BLUR_PROB, d.DEGRADE2_BLUR_SIGMA, d.DEGRADE2_FAMILY_PROB, d.DEGRADE2_BETA_GAUSSIAN, d.DEGRADE2_BETA_PLATEAU,
                   d.DEGRADE2_SINC_PROB, d.DEGRADE2_NOISE_PROB, d.DEGRADE2_NOISE_SIGMA, d.DEGRADE2_SHOT, d.DEGRADE2_SHOT_PROB,
                   d.DEGRADE2_GRAY_PROB, d.DEGRADE2_FINAL_SINC_PROB, d.DEGRADE2_OMEGA, d.DEGRADE2_SINC_FIRST_PROB,
                   tuple(d.DEGRADE2_JPEG_QUALITY), d.DEGRADE2_JPEG_PROB, d.DEGRADE2_KSIZE, d.DEGRADE2_BANK_SIZE,
                   d.DEGRADE2_SINC_BANK_SIZE, d.get("DEGRADE_JPEG_CHROMA", "420"),
                   tuple(d.get("DEGRADE2_RESIZE_PROB", (0.3, 0.4, 0.3))) if d.get("DEGRADE2_RESIZE", False) else None,
                   tuple(d.get("DEGRADE2_RESIZE_RANGE", (0.3, 1.2))),
                   tuple(d.get("DEGRADE2_RESIZE_MODES", ("area", "bilinear", "bicubic"))))


def second_order(lr: Tensor, rows: Tensor, bank: Tensor | None, jpeg_chroma: str | None = "420", out: Tensor | None = None,
                 scratch=None, resize_rows: Tensor | None = None) -> Tensor:
    """The second stage on an LR batch on the 1/255 grid, as the loader issues it: filter2d with rows[0] (blur 2, noise 2), filter2d
    with rows[1] (the final sinc before JPEG), jpeg with rows[2] (jpeg_chroma None: no such launch), filter2d with rows[3] (the final
    sinc after it).  rows: int32 [4, B, 8] on lr's device (SecondOrder.draw).  The last launch writes `out`; scratch: two buffers of
    lr's shape for the passes between (allocated when None: lr is then left as it is; the second may be lr itself, as the loader has
    it, and lr is then overwritten).
    resize_rows: int32 [B, 8] on lr's device (SecondOrder.draw_resize): five launches - filter2d with rows[0] UNQUANTISED (blur 2
    alone: its noise words are zero), rescale with resize_rows (the resize round trip with noise 2 inside; its clamp and rounding are
    the ones the first launch leaves out), then the three last launches as above, over the same two scratch buffers."""
    a, b = scratch if scratch is not None else (torch.empty_like(lr, memory_format=torch.contiguous_format) for _ in range(2))
    if resize_rows is not None:
        filter2d(lr, rows[0], bank, quantise=False, out=a)
        rescale(a, resize_rows, out=b)
        filter2d(b, rows[1], bank, out=a)
        if jpeg_chroma is not None:
            jpeg(a, rows[2], jpeg_chroma, out=a)
        return filter2d(a, rows[3], bank, out=out)
    filter2d(lr, rows[0], bank, out=a)
    filter2d(a, rows[1], bank, out=b)
    if jpeg_chroma is not None:
        jpeg(b, rows[2], jpeg_chroma, out=b)
    return filter2d(b, rows[3], bank, out=out)


class DeviceImageArena:
    """WHOLE training images of any sizes on one device: one packed uint8 arena (HWC/RGB, every image at a 16-byte aligned
    offset) and a device table [N, 3] int64 of (byte offset, H, W).  len() is the number of tiles of the virtual tile list
    (tile_grid: what prepare_dataset.py would have cut), so an epoch has the reference's number of steps and samplers work on
    tile indices; crops() makes (gt, lr) batches from window descriptors with ONE sst_gather_crops launch."""

    def __init__(self, arena: Tensor, table: np.ndarray, crop: int, step: int, upscale: int):
        table = np.asarray(table, np.int64).reshape(-1, 3)
        if arena.dtype != torch.uint8 or arena.dim() != 1 or arena.numel() % 16:
            raise ValueError("DeviceImageArena: the arena must be a flat uint8 tensor of a multiple of 16 bytes")
        if crop <= 0 or crop % 4:
            raise ValueError(f"DeviceImageArena: the crop side must be a positive multiple of 4, got {crop}")
        for off, h, w in table.tolist():
            if off % 16 or off < 0 or h <= 0 or w <= 0 or off + h * w * 3 > arena.numel():
                raise ValueError(f"DeviceImageArena: image (offset {off}, {h}x{w}) is not inside the arena at a 16-byte aligned offset")
        self.arena = arena.contiguous()
        self.device = arena.device
        self.table_host = table
        self.table = torch.from_numpy(table).to(self.device)
        self.crop, self.step, self.upscale = int(crop), int(step), int(upscale)
        self.tiles = tile_grid(table[:, 1:3].tolist(), self.crop, self.step)
        if len(self.tiles) == 0:
            raise ValueError(f"DeviceImageArena: none of the {len(table)} images holds a {crop}x{crop} tile")
        self.lut = lut(self.device)
        self.out = int(self.crop * (1.0 / self.upscale))
        self._bicubic = Bicubic(str(self.device))
        self._span = {}

    def __len__(self) -> int:
        return len(self.tiles)

    @property
    def n_images(self) -> int:
        return len(self.table_host)

    @staticmethod
    def _layout(sizes):
        offs, total = [], 0
        for h, w in sizes:
            offs.append(total)
            total += _pad16(h * w * 3)
        return offs, total

    @classmethod
    def from_arrays(cls, images, crop: int, step: int, upscale: int, device) -> "DeviceImageArena":
        """From uint8 [H, W, 3] arrays (numpy or torch), in the given order."""
        device = torch.device(device)
        arrs = [np.ascontiguousarray(np.asarray(a)) for a in images]
        for i, a in enumerate(arrs):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"DeviceImageArena: image {i} must be uint8 [H, W, 3], got {a.dtype} {a.shape}")
        sizes = [a.shape[:2] for a in arrs]
        offs, total = cls._layout(sizes)
        _check_fits(total, device)
        host = np.zeros(max(total, 16), np.uint8)
        for a, o in zip(arrs, offs):
            host[o:o + a.size] = a.reshape(-1)
        table = np.array([(o, h, w) for o, (h, w) in zip(offs, sizes)], np.int64).reshape(-1, 3)
        return cls(torch.from_numpy(host).to(device), table, crop, step, upscale)

    @classmethod
    def from_dir(cls, image_dir: str, crop: int, step: int, upscale: int, device) -> "DeviceImageArena":
        """Every image under `image_dir` (TrainImageDataset's file list and order), whole.  The sizes are read from the file
        headers first, the arena is sized against the free device memory (MemoryError as for DeviceImageSet), then the images are
        decoded by a thread pool, group by group through one pinned staging buffer, and copied to their places."""
        from PIL import Image
        device = torch.device(device)
        files = TrainImageDataset(image_dir, upscale).image_file_names
        if not files:
            raise ValueError(f"DeviceImageArena: no images under {image_dir}")

        def size(f):
            with Image.open(f) as im:
                return im.size[1], im.size[0]

        with ThreadPoolExecutor(decode_threads()) as pool:
            sizes = list(pool.map(size, files))
            offs, total = cls._layout(sizes)
            _check_fits(total, device)
            arena = torch.zeros(total, dtype=torch.uint8, device=device)
            room = max(_CHUNK_BYTES, max(_pad16(h * w * 3) for h, w in sizes))
            staging = torch.zeros(room, dtype=torch.uint8, pin_memory=device.type == "cuda")
            host = staging.numpy()

            def decode(j, o0):
                a = read_image_hwc(files[j])
                if a.shape != (*sizes[j], 3):
                    raise ValueError(f"DeviceImageArena: {files[j]} decodes to {a.shape}, its header said {sizes[j]}")
                host[offs[j] - o0:offs[j] - o0 + a.size] = a.reshape(-1)

            i0 = 0
            while i0 < len(files):
                i1 = i0 + 1
                while i1 < len(files) and offs[i1] + _pad16(sizes[i1][0] * sizes[i1][1] * 3) - offs[i0] <= room:
                    i1 += 1
                list(pool.map(decode, range(i0, i1), [offs[i0]] * (i1 - i0)))       # re-raises the first failure in file order
                end = offs[i1] if i1 < len(files) else total
                arena[offs[i0]:end].copy_(staging[: end - offs[i0]])                # synchronous: the staging buffer is reused next
                i0 = i1
        table = np.array([(o, h, w) for o, (h, w) in zip(offs, sizes)], np.int64).reshape(-1, 3)
        return cls(arena, table, crop, step, upscale)

    def check_desc(self, desc) -> None:
        """The host-side range check of window descriptors [.., 4] = (image, y0, x0, t): IndexError unless every image exists,
        every window lies inside its image and every t is in 0..7."""
        d = np.asarray(desc, np.int64).reshape(-1, 4)
        if not len(d):
            return
        if d[:, 0].min() < 0 or d[:, 0].max() >= self.n_images:
            raise IndexError(f"DeviceImageArena: a descriptor names an image outside [0, {self.n_images})")
        h, w = self.table_host[d[:, 0], 1], self.table_host[d[:, 0], 2]
        bad = (d[:, 1] < 0) | (d[:, 1] + self.crop > h) | (d[:, 2] < 0) | (d[:, 2] + self.crop > w)
        if bad.any():
            k = int(np.argmax(bad))
            raise IndexError(f"DeviceImageArena: window (y0 {d[k, 1]}, x0 {d[k, 2]}, side {self.crop}) is outside image {d[k, 0]} "
                             f"({h[k]}x{w[k]})")
        if d[:, 3].min() < 0 or d[:, 3].max() > 7:
            raise IndexError("DeviceImageArena: a descriptor's transform is outside 0..7")

    def span(self, with_gt: bool, with_lr: bool) -> int:
        """The most consecutive crop rows one workgroup of the kernel stages: over the bands (LR rows; groups of four rows without
        lr), the extent of the band's tap rows and, with gt, of its own rows."""
        key = (with_gt, with_lr)
        if key not in self._span:
            S = self.crop
            if with_lr:
                _, iy, _, _ = self._bicubic.tables(S, S, 1.0 / self.upscale, "cpu")
                lo, hi = iy.min(1).values.numpy(), iy.max(1).values.numpy()
                if with_gt:
                    b = np.arange(self.out, dtype=np.int64)
                    lo, hi = np.minimum(lo, b * S // self.out), np.maximum(hi, (b + 1) * S // self.out - 1)
                self._span[key] = int((hi - lo).max()) + 1
            else:
                nband = (S + 3) // 4
                self._span[key] = (S + nband - 1) // nband
        return self._span[key]

    def crops(self, desc: Tensor, gt_out: Tensor | None = None, lr_out: Tensor | None = None, with_gt: bool = True,
              with_lr: bool = True, deg: Tensor | None = None, ksize: int | None = None, quantise: bool = True,
              jpeg_chroma: str | None = None):
        """ONE sst_gather_crops launch on the current stream: gt [B,3,S,S] = the windows desc names, transformed, on the 1/255
        grid; lr [B,3,S/up,S/up] = their bicubic.  desc: int32 [B,4] on the arena's device (checked on the host by DeviceCropLoader /
        check_desc).  Writes into gt_out / lr_out when given; with_gt / with_lr = False skips that output (returned as None).
        deg: int32 [B,8] on the device (Degradation.draw) makes it ONE sst_gather_crops_degraded launch instead: the same gt, and lr
        = degrade(gt, deg, upscale, ksize, quantise) bit for bit (blur, bicubic, noise, quantise); ksize defaults to 21.
        jpeg_chroma ('444' / '420', with deg): a second launch, sst_jpeg on lr in place, as degrade(..., jpeg_chroma=) does."""
        if jpeg_chroma is not None:
            _chroma(jpeg_chroma, "DeviceImageArena.crops")
            if deg is None or not quantise:
                raise ValueError("DeviceImageArena.crops: jpeg_chroma needs deg (the qualities are word 6 of its rows) and quantise=True")
        if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 4 or desc.device != self.device:
            raise ValueError(f"DeviceImageArena.crops: desc must be int32 [B, 4] on {self.device}")
        B, S, o = desc.shape[0], self.crop, self.out
        gt = lr = None
        if with_gt:
            gt = gt_out if gt_out is not None else torch.empty(B, 3, S, S, device=self.device)
            _expect(gt, (B, 3, S, S), "gt_out")
        wy = iy = wx = ix = None
        Ty = Tx = 0
        if with_lr:
            lr = lr_out if lr_out is not None else torch.empty(B, 3, o, o, device=self.device)
            _expect(lr, (B, 3, o, o), "lr_out")
            wy, iy, wx, ix = self._bicubic.tables_i32(S, S, 1.0 / self.upscale, self.device)
            Ty, Tx = wy.shape[1], wx.shape[1]
        if deg is not None:
            if not with_lr:
                raise ValueError("DeviceImageArena.crops: deg degrades the lr output; with_lr=False leaves nothing to degrade")
            _check_deg(deg, B, self.device, "DeviceImageArena.crops")
            _abi.check(_abi.lib().sst_gather_crops_degraded(
                _abi.ptr(self.arena), self.arena.numel(), _abi.ptr(self.table), self.n_images, _abi.ptr(desc), B, S, _abi.ptr(self.lut),
                _abi.ptr(gt), _abi.ptr(lr), _abi.ptr(wy), _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), o, o, Ty, Tx,
                self.span(with_gt, True), _abi.ptr(deg), 21 if ksize is None else int(ksize), int(bool(quantise)),
                _abi.stream_ptr()), "sst_gather_crops_degraded")
            if jpeg_chroma is not None:
                jpeg(lr, deg, jpeg_chroma, out=lr)
            return gt, lr
        _abi.check(_abi.lib().sst_gather_crops(_abi.ptr(self.arena), self.arena.numel(), _abi.ptr(self.table), self.n_images,
                                               _abi.ptr(desc), B, S, _abi.ptr(self.lut), _abi.ptr(gt), _abi.ptr(lr), _abi.ptr(wy),
                                               _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), o, o, Ty, Tx,
                                               self.span(with_gt, with_lr), _abi.stream_ptr()), "sst_gather_crops")
        return gt, lr


class DeviceCropLoader:
    """DeviceLoader's semantics (drop_last, bind(), plan() with the range check on the host, one non-blocking upload per epoch) over
    a DeviceImageArena.  The sampler draws TILE indices; plan() turns its order into window descriptors (image, y0, x0, t):
      * as they are, t = 0: the tile grid, i.e. the batches DeviceLoader makes from the pre-cut tiles;
      * random_crop: each tile's (y0, x0) is replaced by a uniform position in the SAME image (images stay drawn in proportion to
        their tile counts);  augment: t uniform in 0..7.
    The draws come from a private torch.Generator seeded from (seed, epoch) and are made for ALL tiles of the set, then indexed by
    the sampler's order: a tile's window and transform in an epoch depend on neither world size nor rank nor batch size, and the
    default CPU generator (model init, shuffles) is never touched.  With both switches off nothing is drawn.  The epoch advances
    with every __iter__; set_epoch() sets it.
    degradation: every batch is one sst_gather_crops_degraded launch; the epoch's deg rows are drawn for ALL tiles as well, from a
    SECOND private generator (seed, epoch and a constant of its own), so a tile's degradation depends on neither world size nor rank
    nor batch size either, the window and transform draws are the ones made without it, and resuming at an epoch reproduces it.
    A degradation that can draw a JPEG quality (Degradation.has_jpeg) adds one sst_jpeg launch per batch; any other leaves the
    launches as they are.
    second (needs degradation): the second-order stage follows, per batch three sst_filter2d launches and one sst_jpeg between the
    last two (second_order()); the gather then writes a scratch buffer of the loader and the last launch the bound lr buffer.  The
    epoch's kernel bank is a function of (seed, epoch); the epoch's rows are drawn for ALL tiles from a THIRD private generator (seed,
    epoch and a constant of its own), so a tile's second stage depends on neither world size nor rank nor batch size, the window,
    transform and first-stage draws are the ones made without it, and resuming at an epoch reproduces it.
    A second stage that resizes (SecondOrder(resize_prob=...)) adds one sst_rescale launch per batch behind the first sst_filter2d;
    the epoch's resize rows are drawn for ALL tiles from a FOURTH private generator (seed, epoch and a constant of its own), so a
    tile's resize depends on neither world size nor rank nor batch size, the window, transform, first-stage, second-stage and bank
    draws are the ones made without it, and resuming at an epoch reproduces it: nothing new goes into a checkpoint.
    A degradation that resizes (Degradation(resize_prob=...)) makes the first stage three launches per batch instead of the one: the
    plain gather (gt alone), sst_blur on gt into a scratch buffer of the loader, and sst_rescale_to from it into the buffer the fused
    gather would have written; the epoch's rows for it are drawn for ALL tiles from a FIFTH private generator (seed, epoch and a
    constant of its own) and carry the noise words and keys of the tile's deg row, so every other draw is the one made without it, a
    tile's resize depends on neither world size nor rank nor batch size, and resuming at an epoch reproduces it."""

    def __init__(self, arena: DeviceImageArena, batch_size: int, sampler=None, random_crop: bool = False, augment: bool = False,
                 seed: int = 0, degradation: Degradation | None = None, second: SecondOrder | None = None):
        if batch_size <= 0:
            raise ValueError("DeviceCropLoader: batch_size must be positive")
        self.dset = arena
        self.batch_size = int(batch_size)
        self.sampler = sampler if sampler is not None else torch.utils.data.RandomSampler(arena)
        self.random_crop, self.augment, self.seed = bool(random_crop), bool(augment), int(seed)
        self.degradation = degradation
        if degradation is not None and degradation.ksize // 2 >= arena.crop:
            raise ValueError(f"DeviceCropLoader: the blur's half window {degradation.ksize // 2} must be smaller than the crop "
                             f"side {arena.crop}")
        self.second = second
        if second is not None:
            if degradation is None:
                raise ValueError("DeviceCropLoader: second (the second-order stage) needs degradation: it works on the first stage's "
                                 "quantised LR batch")
            if second.ksize // 2 >= arena.out:
                raise ValueError(f"DeviceCropLoader: the second stage's half window {second.ksize // 2} must be smaller than the LR "
                                 f"side {arena.out}")
        self.epoch = 0
        self._gt = self._lr = None
        self._scratch = None
        self._hr = None

    def __len__(self) -> int:
        return len(self.sampler) // self.batch_size

    def bind(self, gt: Tensor | None, lr: Tensor | None) -> None:
        """Later batches land in these buffers (the engine's static inputs: the step then copies nothing)."""
        self._gt, self._lr = gt, lr

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def draws(self, epoch: int) -> np.ndarray:
        """The epoch's descriptor of EVERY tile of the set: int32 [len(arena), 4]."""
        a = self.dset
        d = np.zeros((len(a), 4), np.int32)
        d[:, :3] = a.tiles
        if self.random_crop or self.augment:
            g = torch.Generator().manual_seed((self.seed * 1000003 + epoch) % (1 << 63))
            if self.random_crop:
                room = torch.from_numpy(a.table_host[a.tiles[:, 0], 1:3] - a.crop + 1)        # [M, 2] positions per axis, >= 1
                d[:, 1:3] = (torch.randint(0, 1 << 62, room.shape, generator=g, dtype=torch.int64) % room).numpy()
            if self.augment:
                d[:, 3] = torch.randint(0, 8, (len(a),), generator=g, dtype=torch.int64).numpy()
        return d

    def deg_draws(self, epoch: int) -> np.ndarray | None:
        """The epoch's deg row of EVERY tile of the set: int32 [len(arena), 8]; None without a degradation."""
        if self.degradation is None:
            return None
        g = torch.Generator().manual_seed((self.seed * 1000003 + epoch + _DEGRADE_STREAM) % (1 << 63))
        return self.degradation.draw(len(self.dset), g).numpy()

    def second_draws(self, epoch: int):
        """The epoch's second-stage rows of EVERY tile of the set, int32 [4, len(arena), 8] (SecondOrder.draw), and its kernel bank,
        fp32 [M, K, K]; None without a second stage."""
        if self.second is None:
            return None
        base = self.seed * 1000003 + epoch
        rows = self.second.draw(len(self.dset), torch.Generator().manual_seed((base + _SECOND_STREAM) % (1 << 63))).numpy()
        return rows, self.second.draw_bank(torch.Generator().manual_seed((base + _SECOND_BANK_STREAM) % (1 << 63)))

    def resize_draws(self, epoch: int) -> np.ndarray | None:
        """The epoch's resize row of EVERY tile of the set, int32 [len(arena), 8] (SecondOrder.draw_resize); None without a second stage
        that resizes.  The sizes and modes come from a FOURTH private generator (seed, epoch and a constant of its own); the noise
        words are the ones the third generator draws for pass A, which second_draws() then hands out zeroed."""
        if self.second is None or not self.second.has_resize:
            return None
        base, n, o = self.seed * 1000003 + epoch, len(self.dset), self.dset.out
        full = self.second.draw(n, torch.Generator().manual_seed((base + _SECOND_STREAM) % (1 << 63)), keep_noise=True).numpy()
        return self.second.draw_resize(n, o, o, torch.Generator().manual_seed((base + _RESIZE_STREAM) % (1 << 63)), noise=full[0]).numpy()

    def resize1_draws(self, epoch: int) -> np.ndarray | None:
        """The epoch's first-stage resize row of EVERY tile of the set, int32 [len(arena), 8] (Degradation.draw_resize); None without
        a degradation that resizes.  The sizes and modes come from a FIFTH private generator (seed, epoch and a constant of its
        own); the noise word and the key are the ones of the tile's deg row (deg_draws)."""
        if self.degradation is None or not self.degradation.has_resize:
            return None
        n, S = len(self.dset), self.dset.crop
        g = torch.Generator().manual_seed((self.seed * 1000003 + epoch + _RESIZE1_STREAM) % (1 << 63))
        return self.degradation.draw_resize(n, S, S, g, deg_rows=self.deg_draws(epoch)).numpy()

    def plan_all(self):
        """plan_both() and, in the same order, the second stage's rows int32 [4, len(self) * batch_size, 8] and bank (or None, None)."""
        return self.plan_resize()[:4]

    def plan_resize(self):
        """plan_all() and, in the same order (ONE walk of the sampler for all five), the resize rows int32 [len(self) * batch_size, 8],
        or None without a second stage that resizes."""
        return self.plan_first_resize()[:5]

    def plan_first_resize(self):
        """plan_resize() and, in the same order (ONE walk of the sampler for all six), the first-stage resize rows int32
        [len(self) * batch_size, 8], or None without a degradation that resizes."""
        order = np.fromiter(iter(self.sampler), dtype=np.int64)[: len(self) * self.batch_size]
        desc, deg = self._plan(order)
        first = self.resize1_draws(self.epoch)
        first = None if first is None else torch.from_numpy(np.ascontiguousarray(first[order]))
        if self.second is None:
            return desc, deg, None, None, None, first
        rows, bank = self.second_draws(self.epoch)
        resize = self.resize_draws(self.epoch)
        return (desc, deg, torch.from_numpy(np.ascontiguousarray(rows[:, order])), torch.from_numpy(bank),
                None if resize is None else torch.from_numpy(np.ascontiguousarray(resize[order])), first)

    def plan_both(self):
        """The current epoch on the host, in the sampler's order (ONE walk of the sampler): the descriptors int32
        [len(self) * batch_size, 4], tile indices and windows checked against the set, and the deg rows int32 [.., 8] or None."""
        return self._plan(np.fromiter(iter(self.sampler), dtype=np.int64)[: len(self) * self.batch_size])

    def _plan(self, order):
        n = len(self.dset)
        if order.size and (int(order.min()) < 0 or int(order.max()) >= n):
            raise IndexError(f"DeviceCropLoader: the sampler produced an index outside [0, {n})")
        desc = self.draws(self.epoch)[order]
        self.dset.check_desc(desc)
        deg = self.deg_draws(self.epoch)
        return (torch.from_numpy(np.ascontiguousarray(desc)),
                None if deg is None else torch.from_numpy(np.ascontiguousarray(deg[order])))

    def plan(self) -> Tensor:
        """plan_both()'s descriptors."""
        return self.plan_both()[0]

    def __iter__(self):
        B = self.batch_size
        host_first = None
        if self.degradation is not None and self.degradation.has_resize:
            host, host_deg, host_rows, host_bank, host_resize, host_first = self.plan_first_resize()
        else:
            host, host_deg, host_rows, host_bank, host_resize = (self.plan_resize() if self.second is not None
                                                                 else (*self.plan_both(), None, None, None))
        self.epoch += 1
        dev = self.dset.device
        up = (lambda t: t.pin_memory().to(dev, non_blocking=True)) if dev.type == "cuda" else (lambda t: t)
        desc = up(host)
        if host_deg is None:
            for k in range(len(self)):
                yield self.dset.crops(desc[k * B:(k + 1) * B], self._gt, self._lr)
            return
        deg = up(host_deg)                                               # once per epoch, next to desc
        jpeg_chroma = self.degradation.jpeg_chroma if self.degradation.has_jpeg else None
        first = None if host_first is None else up(host_first)
        if self.second is not None:
            yield from self._iter_second(desc, deg, jpeg_chroma, up(host_rows), up(host_bank) if host_bank.numel() else None,
                                         None if host_resize is None else up(host_resize), first)
            return
        for k in range(len(self)):
            sl = slice(k * B, (k + 1) * B)
            yield self._first(desc[sl], deg[sl], None if first is None else first[sl], self._lr, jpeg_chroma)

    def _first(self, desc, deg, first, lr_out, jpeg_chroma):
        """The first stage of one batch into lr_out (None: a new tensor) -> gt, lr.  first None: the fused degraded gather (and its
        sst_jpeg).  first (the batch's first-stage resize rows): the plain gather, gt alone; sst_blur on gt into the loader's HR
        scratch; sst_rescale_to from it to the LR size, with the noise in its rows; then the same sst_jpeg."""
        if first is None:
            return self.dset.crops(desc, self._gt, lr_out, deg=deg, ksize=self.degradation.ksize, jpeg_chroma=jpeg_chroma)
        B, S, o, dev = desc.shape[0], self.dset.crop, self.dset.out, self.dset.device
        gt, _ = self.dset.crops(desc, self._gt, with_lr=False)
        if self._hr is None or self._hr.shape[0] != B:
            self._hr = torch.empty(B, 3, S, S, device=dev)
        if lr_out is not None:
            _expect(lr_out, (B, 3, o, o), "lr_out")
        lr = rescale_to(blur(gt, deg, self.degradation.ksize, out=self._hr), first, (o, o), out=lr_out)
        if jpeg_chroma is not None:
            jpeg(lr, deg, jpeg_chroma, out=lr)
        return gt, lr

    def _iter_second(self, desc, deg, jpeg_chroma, rows, bank, resize=None, first=None):
        """The batches with the second stage: the gather (and its sst_jpeg) into a scratch buffer, then second_order() from it, the last
        launch into the bound lr buffer - no copy.  resize: the epoch's resize rows (one more launch, sst_rescale, per batch).  first:
        the epoch's first-stage resize rows (_first: three launches in the gather's place, into the same scratch buffer)."""
        B, o, dev = self.batch_size, self.dset.out, self.dset.device
        if self._scratch is None or self._scratch[0].shape[0] != B:
            self._scratch = (torch.empty(B, 3, o, o, device=dev), torch.empty(B, 3, o, o, device=dev))
        s0, s1 = self._scratch
        chroma2 = self.second.jpeg_chroma if self.second.has_jpeg else None
        for k in range(len(self)):
            sl = slice(k * B, (k + 1) * B)
            gt, _ = self._first(desc[sl], deg[sl], None if first is None else first[sl], s0, jpeg_chroma)
            lr = self._lr if self._lr is not None else torch.empty(B, 3, o, o, device=dev)
            _expect(lr, (B, 3, o, o), "lr_out")
            yield gt, second_order(s0, rows[:, sl], bank, chroma2, out=lr, scratch=(s1, s0),
                                   resize_rows=None if resize is None else resize[sl])


def check_switches(config) -> None:
    """DATA.RANDOM_CROP, DATA.AUGMENT and DATA.DEGRADE are made by the whole-image gather only; DATA.DEGRADE_JPEG_PROB and
    DATA.DEGRADE_SECOND and DATA.DEGRADE_RESIZE follow DATA.DEGRADE; DATA.DEGRADE2_RESIZE follows DATA.DEGRADE_SECOND."""
    data = config.DATA
    if data.get("DEGRADE", False) and not data.get("ON_DEVICE_WHOLE_IMAGES", False):
        raise ValueError("DATA.DEGRADE needs DATA.ON_DEVICE_WHOLE_IMAGES = True: the per-sample blur and noise are made by the "
                         "whole-image gather (device_data.DeviceCropLoader, sst_gather_crops_degraded), neither the pre-cut crops "
                         "(DATA.ON_DEVICE) nor the host DataLoader have them")
    if data.get("DEGRADE_JPEG_PROB", 0.0) > 0 and not data.get("DEGRADE", False):
        raise ValueError("DATA.DEGRADE_JPEG_PROB needs DATA.DEGRADE = True: the JPEG stage follows the degraded gather and reads its "
                         "quality from the same per-sample rows (set DEGRADE_BLUR_PROB = DEGRADE_NOISE_PROB = 0 for JPEG alone)")
    if data.get("DEGRADE_SECOND", False) and not data.get("DEGRADE", False):
        raise ValueError("DATA.DEGRADE_SECOND needs DATA.DEGRADE = True: the second-order stage (sst_filter2d, DESIGN.md section 23) works "
                         "on the first stage's quantised LR batch (set DEGRADE_BLUR_PROB = DEGRADE_NOISE_PROB = 0 for the second "
                         "stage alone)")
    if data.get("DEGRADE_RESIZE", False) and not data.get("DEGRADE", False):
        raise ValueError("DATA.DEGRADE_RESIZE needs DATA.DEGRADE = True: the first stage's random resize (sst_blur, sst_rescale_to, "
                         "DESIGN.md section 25) sits between that stage's blur and its noise and takes both from the same per-sample "
                         "rows (set DEGRADE_BLUR_PROB = DEGRADE_NOISE_PROB = 0 for the resize alone)")
    if data.get("DEGRADE2_RESIZE", False) and not data.get("DEGRADE_SECOND", False):
        raise ValueError("DATA.DEGRADE2_RESIZE needs DATA.DEGRADE_SECOND = True: the random resize round trip (sst_rescale, DESIGN.md "
                         "section 24) is a pass of the second-order stage, between its blur and its final sinc / JPEG")
    if (data.get("RANDOM_CROP", False) or data.get("AUGMENT", False)) and not data.get("ON_DEVICE_WHOLE_IMAGES", False):
        raise ValueError("DATA.RANDOM_CROP / DATA.AUGMENT need DATA.ON_DEVICE_WHOLE_IMAGES = True: the random window and the flips / "
                         "transposition are made by the whole-image gather (device_data.DeviceCropLoader), no other data path has them")


def announce_degradation(config, degradation: Degradation, second: SecondOrder | None = None) -> None:
    """The drivers' one log line for DATA.DEGRADE (one more with a JPEG stage, one more with the second-order stage, one more with its resize), and a warning
    for every configured BackProjectionLoss(target="gt"): its target is the bicubic of gt, which is then not the LR image the generator
    saw (target="lr" takes the loader's)."""
    import warnings
    from .loss import BackProjectionLoss
    print(f"[Data] DATA.DEGRADE: lr = quantise(clamp(bicubic(gt * k) + n)) per sample in the gather launch, {degradation!r}")
    if degradation.has_resize:
        print("[Data] DATA.DEGRADE_RESIZE: instead lr = quantise(clamp(resize(resize(gt * k) + n))) per sample, to a size of its own, n "
              "there, then to the LR size, no antialias (plain gather, sst_blur, sst_rescale_to: three launches for the one)"
              + ("" if degradation._fixed else f": (up, down, keep) = {degradation.resize_prob}, scale in {degradation.resize_range}, "
                                               f"modes {degradation.resize_modes}"))
    if degradation.has_jpeg:
        print(f"[Data] DATA.DEGRADE: then lr = jpeg(lr) in a second launch (sst_jpeg, integer codec, chroma {degradation.jpeg_chroma})"
              + ("" if degradation._fixed else f": quality uniform in {degradation.jpeg_quality} with probability {degradation.jpeg_prob:g}"))
    if second is not None:
        print("[Data] DATA.DEGRADE_SECOND: then lr = sinc(jpeg(sinc(quantise(clamp(lr * k2 + n2))))) per sample (sst_filter2d x 3 around "
              f"sst_jpeg, kernels from a table drawn per epoch), {second!r}")
        if second.has_resize:
            print("[Data] DATA.DEGRADE2_RESIZE: with lr * k2 unquantised, then resize to a size per sample, n2 there, resize back, clamp, "
                  "quantise (sst_rescale, one more launch between the first two sst_filter2d)"
                  + ("" if second._fixed else f": (up, down, keep) = {second.resize_prob}, scale in {second.resize_range}, "
                                              f"modes {second.resize_modes}"))
    loss = config.MODEL.G_LOSS
    for where in ("CRITERIONS", "WARMUP_CRITERIONS"):
        for name, crit in loss.get(where, {}).items():
            if isinstance(crit, BackProjectionLoss) and crit.target == "gt":
                warnings.warn(f"DATA.DEGRADE: MODEL.G_LOSS.{where}[{name!r}] is a BackProjectionLoss(target='gt'); its target is the "
                              "bicubic of gt, not the degraded LR image the generator is given")


def on_device(config) -> bool:
    """The drivers' switch: True when the batches come from device memory (DATA.ON_DEVICE or DATA.ON_DEVICE_WHOLE_IMAGES)."""
    check_switches(config)
    return bool(config.DATA.ON_DEVICE or config.DATA.get("ON_DEVICE_WHOLE_IMAGES", False))


def train_loader(config, train_dataset, world: int, rank: int):
    """The drivers' device data path: (loader, sampler or None).  DATA.ON_DEVICE: a DeviceLoader over the pre-cut crops, from
    `train_dataset` when one is given (from_dataset), else from DATA.TRAIN_GT_IMAGES_DIR (from_dir).  DATA.ON_DEVICE_WHOLE_IMAGES:
    a DeviceCropLoader over the whole images of DATA.TRAIN_ORIGINAL_IMAGES_DIR (or over `train_dataset` when it is a
    DeviceImageArena).  Data-parallel ranks shard the set with a DistributedSampler."""
    check_switches(config)
    up = config.DATA.UPSCALE_FACTOR
    DS = torch.utils.data.distributed.DistributedSampler
    if config.DATA.get("ON_DEVICE_WHOLE_IMAGES", False):
        if isinstance(train_dataset, DeviceImageArena):
            arena = train_dataset
        elif train_dataset is None:
            arena = DeviceImageArena.from_dir(config.DATA.TRAIN_ORIGINAL_IMAGES_DIR, config.DATA.GT_IMAGE_SIZE, config.DATA.CROP_STEP,
                                              up, config.DEVICE)
        else:
            raise ValueError("DATA.ON_DEVICE_WHOLE_IMAGES: the whole images come from DATA.TRAIN_ORIGINAL_IMAGES_DIR (or a "
                             "DeviceImageArena passed as train_dataset), not from a dataset of crops")
        sampler = DS(arena, world, rank, shuffle=True) if world > 1 else None
        degradation = Degradation.from_config(config)
        loader = DeviceCropLoader(arena, config.DATA.BATCH_SIZE, sampler, config.DATA.RANDOM_CROP, config.DATA.AUGMENT,
                                  config.DATA.SEED, degradation, SecondOrder.from_config(config))
        if degradation is not None and rank == 0:
            announce_degradation(config, degradation, loader.second)
        loader.set_epoch(config.EXP.START_EPOCH)
        return loader, sampler
    if train_dataset is not None:
        dset = DeviceImageSet.from_dataset(train_dataset, up, config.DEVICE)
    else:
        dset = DeviceImageSet.from_dir(config.DATA.TRAIN_GT_IMAGES_DIR, up, config.DEVICE)
    sampler = DS(dset, world, rank, shuffle=True) if world > 1 else None
    return DeviceLoader(dset, config.DATA.BATCH_SIZE, sampler), sampler
