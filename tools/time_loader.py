#!/usr/bin/env python3
"""Rate of train() by data path, B = 16, 96-px crops, full-size SRGAN (G 64 ch x 16 blocks, D 64 ch; adversarial + MSE + structure
tensor / 3, D updated every step - bench.py's workload):

    device tensors   the engine stepped on pre-made device tensors (the rate the kernels can take; no loader at all)
    host             train() with the host DataLoader (PIL decode + CPU Bicubic in one worker, pinned H2D copy)
    host+lr_dev      the same with KERNEL.LR_ON_DEVICE (the LR made on the GPU from the copied GT batch)
    on_device        train() with DATA.ON_DEVICE (device-resident uint8 set, one sst_gather_batch launch per batch)
    whole_images     train() with DATA.ON_DEVICE_WHOLE_IMAGES (whole images of differing sizes in device memory, one
                     sst_gather_crops launch per batch; the tile grid, no transform)
    whole_images_aug the same with DATA.RANDOM_CROP and DATA.AUGMENT

M synthetic crops on the 1/255 grid are written as PNGs into a temporary directory first; train() reads them from there
(DATA.TRAIN_GT_IMAGES_DIR).  The whole_images legs read a second synthetic set, DIV2K-shaped whole images of four different
sizes with at least as many 96-px tiles (DATA.TRAIN_ORIGINAL_IMAGES_DIR).  A step's time is taken over steps [S0, S0 + S) of one epoch, with a device sync at both ends only.
The one-time decode + upload of the on_device set and of the whole-image arena are timed separately.  --repeat R runs the
chosen legs R times, round robin, and reports every repeat (the spread among the repeats of one leg is the yardstick for a
difference between two legs).  Prints one JSON line.

    python tools/time_loader.py [--images M] [--steps S] [--skip S0] [--repeat R]
                                [--cases device,host,host_lr,on_device,whole_images,whole_images_aug]
    python tools/time_loader.py --gather-only [--iters N]     # N gather launches alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d OUT -o gather -- python tools/time_loader.py --gather-only
    python tools/time_loader.py --gather-only --crops grid|odd_x0|transposed [--iters N]
        # the same trace with N sst_gather_crops launches beside N sst_gather_batch launches on the same tiles, in one process
    python tools/time_loader.py degrade [--launches L] [--replays R] [--repeat N] [--parent-lib PATH]
        # the degradation stage (DATA.DEGRADE), B = 16, S = 96, x4, us per batch: each leg is a hipGraph of L launches on L different
        # batches (random windows, all transforms), replayed R times between two device events; the legs run round robin N times and
        # every repeat is reported.  Legs: the plain sst_gather_crops (and, with --parent-lib, the same launch through another build of
        # the library, e.g. the parent commit's, in the same process); sst_gather_crops_degraded at K = 7 and 21 with and without
        # noise; and the same degradation as fp32 torch ops on the gathered gt (reflect pad, per-sample grouped conv2d with
        # precomputed weights, Bicubic("cuda"), randn, clamp, round) - the yardstick
    python tools/time_loader.py jpeg [--launches L] [--replays R] [--repeat N] [--parent-lib PATH [--parent-first]]
        # the JPEG stage (DATA.DEGRADE_JPEG_PROB), same sizes and method, every sample with blur (K = 21), noise and a quality in
        # 30..95.  Legs: sst_gather_crops_degraded alone (and, with --parent-lib, through another build of the library in the same
        # process); the same followed by sst_jpeg in 444 and in 420; sst_jpeg alone on the LR buffer; and the degraded gather followed
        # by the same codec as torch int32 ops on the device (torch_jpeg, checked against the kernel bit for bit first) - the yardstick
    python tools/time_loader.py second [--launches L] [--replays R] [--repeat N] [--parent-lib PATH [--parent-first]]
        # the second-order stage (DATA.DEGRADE_SECOND), same sizes and method, every sample with all stages on (first stage: blur
        # K = 21, noise, JPEG 420; second stage: blur 2, noise 2, the final sinc, JPEG).  Legs: the off path = the degraded gather and
        # its sst_jpeg (and, with --parent-lib, the same two launches through another build of the library in the same process); each
        # added launch alone on the LR buffers (pass A, pass B, the second sst_jpeg, pass C); the whole second-order batch as the
        # loader issues it; and the same pipeline behind the same first stage as torch ops (F.pad(reflect), grouped conv2d with the
        # per-sample weights, randn, clamp, round, torch_jpeg) - the yardstick
    python tools/time_loader.py resize [--launches L] [--replays R] [--repeat N] [--parent-lib PATH [--parent-first]]
        # the resize round trip inside the second-order stage (DATA.DEGRADE2_RESIZE), same sizes and method, every sample with all
        # stages on.  Legs: the off path = the degraded gather and the second-order batch without resize (and, with --parent-lib,
        # the same six launches through another build of the library in the same process); sst_rescale alone on the LR buffers with
        # every sample at the scale 0.3, 1.0 and 1.2 and with the drawn rows (up, down, keep = 0.3, 0.4, 0.3); pass A unquantised;
        # the whole batch with resize on; and the drawn round trips as torch ops - one F.interpolate pair PER SAMPLE, since the
        # intermediate sizes differ per sample, with randn noise between them - the yardstick for sst_rescale alone
    python tools/time_loader.py resize1 [--launches L] [--replays R] [--repeat N] [--parent-lib PATH [--parent-first]]
        # the first stage's random resize (DATA.DEGRADE_RESIZE), same sizes and method, every sample with blur (K = 21) and noise.
        # Legs: the off path = the fused sst_gather_crops_degraded (and, with --parent-lib, the same launch through another build of
        # the library in the same process); the plain gather writing gt alone; sst_blur alone; sst_rescale_to alone on the blurred
        # batch with every sample at the scale 0.15, 1.0 and 1.5 and with the drawn rows (up, down, keep = 0.2, 0.7, 0.1); the whole
        # three-launch first stage; and the same stage as torch ops behind the plain gather (reflect pad, grouped conv2d, one
        # F.interpolate pair PER SAMPLE with randn noise between them, clamp, round) - the yardstick
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import Dataset  # noqa: E402

B, HR, UP = 16, 96, 4


def write_crops(d, m, seed=0):
    """m DIV2K-like 96-px crops (bicubic-upsampled coarse noise, as dataset.SyntheticImageDataset 'lowfreq') on the 1/255 grid."""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    for i0 in range(0, m, 256):
        n = min(256, m - i0)
        base = torch.rand(n, 3, HR // 8, HR // 8, generator=g)
        x = torch.nn.functional.interpolate(base, size=(HR, HR), mode="bicubic", align_corners=False)
        u8 = torch.round(x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        for j in range(n):
            Image.fromarray(np.ascontiguousarray(u8[j])).save(os.path.join(d, f"crop_{i0 + j:06d}.png"))


WHOLE_SIZES = ((1356, 2040), (2040, 1356), (1404, 2039), (1117, 1853))      # H, W: DIV2K-like, two odd widths


def write_whole_images(d, tiles, seed=1):
    """Whole images of WHOLE_SIZES in turn (bicubic-upsampled coarse noise) until they hold at least `tiles` 96-px tiles."""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    have = i = 0
    while have < tiles:
        h, w = WHOLE_SIZES[i % len(WHOLE_SIZES)]
        base = torch.rand(1, 3, h // 8, w // 8, generator=g)
        x = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False)
        u8 = torch.round(x[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        Image.fromarray(u8).save(os.path.join(d, f"whole_{i:04d}.png"), compress_level=1)
        have += (h // HR) * (w // HR)
        i += 1
    return i


class _OnePair(Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(0)
        return torch.rand(3, HR, HR, generator=g), torch.rand(3, HR // UP, HR // UP, generator=g)


def make_cfg(gt_dir, name):
    from srganst.config import Config
    from srganst.loss import MSELoss, StructureTensorLoss
    cfg = Config()
    cfg.EXP.NAME = name
    cfg.EXP.N_EPOCHS = 1
    cfg.DATA.TRAIN_GT_IMAGES_DIR = gt_dir
    cfg.DATA.BATCH_SIZE = B
    cfg.LOG_TRAIN_PERIOD = 1 << 30            # only batch 0 logs (one sync), like any long run between log steps
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1.0 / 3.0)
    cfg.SOLVER.D_UPDATE_INTERVAL = 1
    return cfg


class _Window:
    """Wraps TrainEngine.step: device sync + clock when `skip` and `skip + steps` steps have been issued."""

    def __init__(self, skip, steps):
        from srganst.engine import TrainEngine
        self.cls, self.orig = TrainEngine, TrainEngine.step
        self.skip, self.steps, self.n, self.t = skip, steps, 0, []
        win = self

        def step(eng, gt, lr):
            if win.n in (win.skip, win.skip + win.steps):
                torch.cuda.synchronize()
                win.t.append(time.perf_counter())
            win.n += 1
            return win.orig(eng, gt, lr)
        TrainEngine.step = step

    def close(self):
        self.cls.step = self.orig
        return (self.t[1] - self.t[0]) / self.steps if len(self.t) == 2 else float("nan")


def time_train(gt_dir, name, skip, steps, **switches):
    from srganst.train import train
    cfg = make_cfg(gt_dir, name)
    for k, v in switches.items():
        getattr(cfg, k.split(".")[0])[k.split(".")[1]] = v
    w = _Window(skip, steps)
    try:
        train(cfg, test_dataset=_OnePair(), max_steps_per_epoch=skip + steps + 1)
    finally:
        sec = w.close()
    return sec


def time_device_tensors(gt_dir, skip, steps):
    from srganst.engine import TrainEngine
    from srganst.model import Discriminator, Generator
    cfg = make_cfg(gt_dir, "time_loader_dev_tensors")
    torch.manual_seed(cfg.DATA.SEED)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    eng = TrainEngine(cfg, G, D)
    g = torch.Generator().manual_seed(1)
    gt = (torch.randint(0, 256, (B, 3, HR, HR), generator=g).float() / 255).cuda()
    lr = (torch.randint(0, 256, (B, 3, HR // UP, HR // UP), generator=g).float() / 255).cuda()
    for _ in range(skip):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    eng.close()
    return sec


def gather_only(iters):
    from srganst.device_data import DeviceImageSet, DeviceLoader
    g = torch.Generator().manual_seed(0)
    dset = DeviceImageSet(torch.randint(0, 256, (4096, HR, HR, 3), generator=g, dtype=torch.uint8).cuda(), UP)
    ld = DeviceLoader(dset, B)
    ld.bind(torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, HR // UP, HR // UP, device="cuda"))
    n = 0
    while n < iters:
        for _ in ld:
            n += 1
            if n == iters:
                break
    torch.cuda.synchronize()
    print(json.dumps({"gather_launches": n, "batch": B, "hr": HR}))


def gather_crops_only(iters, case):
    """`iters` sst_gather_crops launches of one kind beside `iters` sst_gather_batch launches on the same tiles (cut from the same
    images on the device), alternating: grid = the tile grid, t = 0; odd_x0 = the same windows moved to an odd x0, t = 0;
    transposed = the grid with t = 5 (transpose + hflip)."""
    from srganst.device_data import DeviceCropLoader, DeviceImageArena, DeviceImageSet
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 4]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    tiles = torch.from_numpy(arena.tiles)
    pick = torch.randperm(len(tiles), generator=g)[:4096]
    store = torch.stack([imgs[n][y:y + HR, x:x + HR] for n, y, x in tiles[pick].tolist()])
    dset = DeviceImageSet(store.cuda(), UP)
    desc = torch.zeros(len(pick), 4, dtype=torch.int32)
    desc[:, :3] = tiles[pick]
    if case == "odd_x0":
        room = torch.from_numpy(arena.table_host[desc[:, 0].long().numpy(), 2]) - HR
        desc[:, 2] = torch.minimum(desc[:, 2] | 1, ((room - 1) | 1).to(torch.int32))
        assert bool((desc[:, 2] % 2 == 1).all())
    elif case == "transposed":
        desc[:, 3] = 5
    elif case != "grid":
        raise SystemExit(f"--crops {case}: grid, odd_x0 or transposed")
    arena.check_desc(desc.numpy())
    desc, idx = desc.cuda(), torch.arange(len(pick), dtype=torch.int32).cuda()
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, HR // UP, HR // UP, device="cuda")
    for n in range(iters):
        k = (n * B) % (len(pick) - B)
        dset.batch(idx[k:k + B], gt, lr)
        arena.crops(desc[k:k + B], gt, lr)
    torch.cuda.synchronize()
    print(json.dumps({"gather_launches_each": iters, "crops_case": case, "batch": B, "hr": HR, "arena_bytes": arena.arena.numel()}))


def degrade_mode(launches, replays, repeat, parent_lib):
    import ctypes
    from srganst import _abi
    from srganst.bicubic import Bicubic
    from srganst.device_data import Degradation, DeviceImageArena, degrade_rows
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 2]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    n = launches * B
    tiles = torch.from_numpy(arena.tiles)[torch.randperm(len(arena), generator=g)[:n]]
    room = torch.from_numpy(arena.table_host[tiles[:, 0].numpy(), 1:3] - HR + 1)
    desc = torch.zeros(n, 4, dtype=torch.int32)
    desc[:, 0] = tiles[:, 0]
    desc[:, 1:3] = (torch.randint(0, 1 << 30, (n, 2), generator=g) % room).to(torch.int32)
    desc[:, 3] = torch.randint(0, 8, (n,), generator=g).to(torch.int32)
    arena.check_desc(desc.numpy())
    desc = desc.cuda()
    draw = lambda noise_prob: Degradation(noise_prob=noise_prob).draw(n, torch.Generator().manual_seed(1)).cuda()
    deg_noise, deg_quiet = draw(1.0), draw(0.0)
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, HR // UP, HR // UP, device="cuda")
    bic = Bicubic("cuda")

    def torch_weights(deg, K):          # per-sample normalised kernels [n * 3, 1, K, K], made beforehand: not part of the timed work
        q = deg[:, :3].contiguous().view(torch.float32).double()
        d = torch.arange(-(K // 2), K // 2 + 1, device="cuda", dtype=torch.float64)
        dy, dx = d[None, :, None], d[None, None, :]
        w = torch.exp(-(q[:, 0, None, None] * dx * dx + q[:, 1, None, None] * dx * dy + q[:, 2, None, None] * dy * dy))
        w = (w / w.sum((1, 2), keepdim=True)).float()
        return w.repeat_interleave(3, 0)[:, None].contiguous()

    def torch_leg(K):
        w, p = torch_weights(deg_noise, K), K // 2
        sn = deg_noise[:, 3].contiguous().view(torch.float32)

        def run(k):
            arena.crops(desc[k * B:(k + 1) * B], gt, lr)
            x = torch.nn.functional.pad(gt, (p, p, p, p), mode="reflect").reshape(1, B * 3, HR + 2 * p, HR + 2 * p)
            x = torch.nn.functional.conv2d(x, w[k * B * 3:(k + 1) * B * 3], groups=B * 3).reshape(B, 3, HR, HR)
            y = bic(x, scale=1.0 / UP) + sn[k * B:(k + 1) * B, None, None, None] * torch.randn(B, 3, HR // UP, HR // UP, device="cuda")
            lr.copy_(torch.round(y.clamp(0, 1) * 255) / 255)
        return run

    def crops_leg(deg, K):
        return lambda k: arena.crops(desc[k * B:(k + 1) * B], gt, lr, deg=deg[k * B:(k + 1) * B], ksize=K)

    legs = {"gather_crops": lambda k: arena.crops(desc[k * B:(k + 1) * B], gt, lr)}
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        other.sst_gather_crops.restype, other.sst_gather_crops.argtypes = _abi.SIGNATURES["sst_gather_crops"]
        wy, iy, wx, ix = arena._bicubic.tables_i32(HR, HR, 1.0 / UP, arena.device)
        o = HR // UP

        def parent(k):
            rc = other.sst_gather_crops(arena.arena.data_ptr(), arena.arena.numel(), arena.table.data_ptr(), arena.n_images,
                                        desc[k * B:(k + 1) * B].data_ptr(), B, HR, arena.lut.data_ptr(), gt.data_ptr(), lr.data_ptr(),
                                        wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), o, o, wy.shape[1], wx.shape[1],
                                        arena.span(True, True), _abi.stream_ptr())
            assert rc == 0, rc
        legs["gather_crops_parent_lib"] = parent
    for K in (7, 21):
        legs[f"degraded_k{K}"] = crops_leg(deg_quiet, K)
        legs[f"degraded_k{K}_noise"] = crops_leg(deg_noise, K)
    for K in (7, 21):
        legs[f"torch_ops_k{K}_noise"] = torch_leg(K)

    graphs = {}
    for name, run in legs.items():
        for k in range(min(3, launches)):               # warm up: tables, code objects, the allocator's pool
            run(k)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for k in range(launches):
                run(k)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    out = {"mode": "degrade", "batch": B, "hr": HR, "scale": UP, "launches_per_graph": launches, "replays": replays, "repeat": repeat,
           "us_per_batch": {name: [] for name in legs}}
    for _ in range(repeat):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                gr.replay()
            t1.record()
            torch.cuda.synchronize()
            out["us_per_batch"][name].append(round(t0.elapsed_time(t1) * 1e3 / (replays * launches), 2))
    out["median_us_per_batch"] = {name: sorted(v)[len(v) // 2] for name, v in out["us_per_batch"].items()}
    print(json.dumps(out))


def torch_jpeg(lr, q_luma, q_chroma, on, chroma, T):
    """The codec of csrc/jpeg.hip as torch int32 ops on the device: lr fp32 [B,3,h,w], q_luma / q_chroma int32
    [B,1,1,8,8] (the samples' tables), on bool [B] (False: the sample keeps its bits), chroma 0 / 1, T int32 [8,8].  The yardstick of
    the jpeg legs, and checked against the kernel bit for bit before anything is timed."""
    n, _, h, w = lr.shape
    M = 16 if chroma else 8
    iy = torch.arange(-(-h // M) * M, device=lr.device).clamp(max=h - 1)
    ix = torch.arange(-(-w // M) * M, device=lr.device).clamp(max=w - 1)
    p = torch.round(255 * lr.clamp(0, 1)).to(torch.int32)[:, :, iy][:, :, :, ix]
    R, G, Bl = p[:, 0], p[:, 1], p[:, 2]
    planes = [(19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16,
              (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16,
              (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16]
    if chroma:
        planes[1:] = [(c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2 for c in planes[1:]]
    Tt = T.t().contiguous()

    def round_trip(pl, q):
        m, k = pl.shape[1] // 8, pl.shape[2] // 8
        s = pl.reshape(n, m, 8, k, 8).permute(0, 1, 3, 2, 4) - 128                      # [n, m, k, y, x]
        a = ((s[..., :, None, :] * T).sum(-1, dtype=torch.int32) + 512) >> 10            # a[y][u] = sum_x T[u][x] s[y][x]
        F = (T[:, :, None] * a[..., None, :, :]).sum(-2, dtype=torch.int32)              # F[v][u] = sum_y T[v][y] a[y][u]
        D = torch.sign(F) * torch.div(F.abs() + q * 32768, q * 65536, rounding_mode="floor") * q
        b = ((Tt[:, :, None] * D[..., None, :, :]).sum(-2, dtype=torch.int32) + 512) >> 10      # b[y][u] = sum_v T[v][y] D[v][u]
        r = ((b[..., :, None, :] * Tt).sum(-1, dtype=torch.int32) + 32768) >> 16         # r[y][x] = sum_u T[u][x] b[y][u]
        return (r + 128).clamp(0, 255).permute(0, 1, 3, 2, 4).reshape(n, m * 8, k * 8)
    Y, cb, cr = round_trip(planes[0], q_luma), round_trip(planes[1], q_chroma), round_trip(planes[2], q_chroma)
    if chroma:
        cb, cr = (c.repeat_interleave(2, 1).repeat_interleave(2, 2) for c in (cb, cr))
    cb, cr = cb - 128, cr - 128
    rgb = torch.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                       Y + ((116130 * cb + 32768) >> 16)], 1).clamp(0, 255)[:, :, :h, :w]
    # (divided by a tensor: by a Python scalar, torch's device kernel multiplies by the rounded reciprocal, which is not p / 255.f)
    return torch.where(on[:, None, None, None], rgb.float() / torch.full((), 255.0, device=lr.device), lr)


def jpeg_mode(launches, replays, repeat, parent_lib, parent_first=False):
    import ctypes
    from srganst import _abi
    from srganst.device_data import JPEG_CHROMA, Degradation, DeviceImageArena, jpeg
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 2]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    n, K, o = launches * B, 21, HR // UP
    tiles = torch.from_numpy(arena.tiles)[torch.randperm(len(arena), generator=g)[:n]]
    room = torch.from_numpy(arena.table_host[tiles[:, 0].numpy(), 1:3] - HR + 1)
    desc = torch.zeros(n, 4, dtype=torch.int32)
    desc[:, 0] = tiles[:, 0]
    desc[:, 1:3] = (torch.randint(0, 1 << 30, (n, 2), generator=g) % room).to(torch.int32)
    desc[:, 3] = torch.randint(0, 8, (n,), generator=g).to(torch.int32)
    arena.check_desc(desc.numpy())
    desc = desc.cuda()
    deg_host = Degradation(jpeg_prob=1.0).draw(n, torch.Generator().manual_seed(1))       # blur, noise and a quality in 30..95 each
    deg = deg_host.cuda()
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, o, o, device="cuda")
    # the comparator's constants, made beforehand: not part of the timed work
    tabs = (ctypes.c_int * 128)()
    q_all = []
    for Q in deg_host[:, 6].tolist():
        _abi.check(_abi.lib().sst_jpeg_tables(Q, tabs), "sst_jpeg_tables")
        q_all.append(list(tabs))
    q_all = torch.tensor(q_all, dtype=torch.int32).reshape(n, 2, 1, 1, 8, 8).cuda()
    on = torch.ones(n, dtype=torch.bool, device="cuda")
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    C = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    C[0] = np.sqrt(0.125)
    T = torch.from_numpy(np.rint(8192 * C).astype(np.int32)).cuda()

    def degraded(k):
        arena.crops(desc[k * B:(k + 1) * B], gt, lr, deg=deg[k * B:(k + 1) * B], ksize=K)

    def with_jpeg(mode):
        return lambda k: arena.crops(desc[k * B:(k + 1) * B], gt, lr, deg=deg[k * B:(k + 1) * B], ksize=K, jpeg_chroma=mode)

    def jpeg_only(mode):
        return lambda k: jpeg(lr, deg[k * B:(k + 1) * B], mode, out=lr)

    def torch_leg(mode):
        def run(k):
            degraded(k)
            lr.copy_(torch_jpeg(lr, q_all[k * B:(k + 1) * B, 0], q_all[k * B:(k + 1) * B, 1], on[k * B:(k + 1) * B], JPEG_CHROMA[mode], T))
        return run

    for mode in ("444", "420"):                          # the comparator is the kernel's codec: the same bits
        with_jpeg(mode)(0)
        want = lr.clone()
        torch_leg(mode)(0)
        assert torch.equal(lr, want), (f"torch_jpeg and sst_jpeg differ ({mode}): {int((lr != want).sum())} of {lr.numel()} elements, "
                                       f"by {float((lr - want).abs().max()) * 255:.3g} levels at most")
    legs = {"degraded_k21_noise": degraded}
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        other.sst_gather_crops_degraded.restype, other.sst_gather_crops_degraded.argtypes = _abi.SIGNATURES["sst_gather_crops_degraded"]
        wy, iy, wx, ix = arena._bicubic.tables_i32(HR, HR, 1.0 / UP, arena.device)

        def parent(k):
            rc = other.sst_gather_crops_degraded(arena.arena.data_ptr(), arena.arena.numel(), arena.table.data_ptr(), arena.n_images,
                                                 desc[k * B:(k + 1) * B].data_ptr(), B, HR, arena.lut.data_ptr(), gt.data_ptr(),
                                                 lr.data_ptr(), wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), o, o,
                                                 wy.shape[1], wx.shape[1], arena.span(True, True), deg[k * B:(k + 1) * B].data_ptr(), K, 1,
                                                 _abi.stream_ptr())
            assert rc == 0, rc
        legs["degraded_k21_noise_parent_lib"] = parent
        if parent_first:                                 # the same two legs in the other order: what the order alone is worth
            legs = {"degraded_k21_noise_parent_lib": parent, "degraded_k21_noise": degraded}
    for mode in ("444", "420"):
        legs[f"degraded_jpeg_{mode}"] = with_jpeg(mode)
    for mode in ("444", "420"):
        legs[f"jpeg_only_{mode}"] = jpeg_only(mode)
    for mode in ("444", "420"):
        legs[f"degraded_torch_ops_jpeg_{mode}"] = torch_leg(mode)

    graphs = {}
    for name, run in legs.items():
        for k in range(min(3, launches)):               # warm up: tables, code objects, the allocator's pool
            run(k)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for k in range(launches):
                run(k)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    out = {"mode": "jpeg", "batch": B, "hr": HR, "scale": UP, "launches_per_graph": launches, "replays": replays, "repeat": repeat,
           "us_per_batch": {name: [] for name in legs}}
    for _ in range(repeat):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                gr.replay()
            t1.record()
            torch.cuda.synchronize()
            out["us_per_batch"][name].append(round(t0.elapsed_time(t1) * 1e3 / (replays * launches), 2))
    out["median_us_per_batch"] = {name: sorted(v)[len(v) // 2] for name, v in out["us_per_batch"].items()}
    print(json.dumps(out))


def second_mode(launches, replays, repeat, parent_lib, parent_first=False):
    import ctypes
    from srganst import _abi
    from srganst.device_data import Degradation, DeviceImageArena, SecondOrder, filter2d, jpeg, second_order
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 2]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    n, K, o = launches * B, 21, HR // UP
    tiles = torch.from_numpy(arena.tiles)[torch.randperm(len(arena), generator=g)[:n]]
    room = torch.from_numpy(arena.table_host[tiles[:, 0].numpy(), 1:3] - HR + 1)
    desc = torch.zeros(n, 4, dtype=torch.int32)
    desc[:, 0] = tiles[:, 0]
    desc[:, 1:3] = (torch.randint(0, 1 << 30, (n, 2), generator=g) % room).to(torch.int32)
    desc[:, 3] = torch.randint(0, 8, (n,), generator=g).to(torch.int32)
    arena.check_desc(desc.numpy())
    desc = desc.cuda()
    deg = Degradation(jpeg_prob=1.0).draw(n, torch.Generator().manual_seed(1)).cuda()
    so = SecondOrder(blur_prob=1.0, noise_prob=1.0, final_sinc_prob=1.0, jpeg_prob=1.0, ksize=K)
    rows_host = so.draw(n, torch.Generator().manual_seed(2))
    bank_host = so.draw_bank(torch.Generator().manual_seed(3))
    rows, bank = rows_host.cuda(), torch.from_numpy(bank_host).cuda()
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, o, o, device="cuda")
    s0, s1 = torch.empty_like(lr), torch.empty_like(lr)
    sl = lambda k: slice(k * B, (k + 1) * B)

    def off(k):
        arena.crops(desc[sl(k)], gt, lr, deg=deg[sl(k)], ksize=K, jpeg_chroma="420")

    def whole(k):
        arena.crops(desc[sl(k)], gt, s0, deg=deg[sl(k)], ksize=K, jpeg_chroma="420")
        second_order(s0, rows[:, sl(k)], bank, "420", out=lr, scratch=(s1, s0))

    # ---- the comparator's constants, made beforehand: not part of the timed work.  A pass a sample does not take (B or C) is the
    # identity kernel there, so that the torch pipeline is the same ops for every sample
    p = K // 2
    ident = torch.zeros(K, K)
    ident[p, p] = 1.0
    table = torch.cat([torch.from_numpy(bank_host), ident[None]]).cuda()
    wts = [table[rows_host[j, :, 0].long()].repeat_interleave(3, 0)[:, None].contiguous() for j in (0, 1, 3)]     # idx -1: the last
    sn, sp = (rows[0, :, j].contiguous().view(torch.float32)[:, None, None, None] for j in (1, 2))
    gray = rows[0, :, 3].bool()[:, None, None, None]
    tabs = (ctypes.c_int * 128)()
    q_all = []
    for Q in rows_host[2, :, 6].tolist():
        _abi.check(_abi.lib().sst_jpeg_tables(Q, tabs), "sst_jpeg_tables")
        q_all.append(list(tabs))
    q_all = torch.tensor(q_all, dtype=torch.int32).reshape(n, 2, 1, 1, 8, 8).cuda()
    on = torch.ones(n, dtype=torch.bool, device="cuda")
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    C = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    C[0] = np.sqrt(0.125)
    T = torch.from_numpy(np.rint(8192 * C).astype(np.int32)).cuda()
    pad, conv2d = torch.nn.functional.pad, torch.nn.functional.conv2d

    def conv(v, w, k):
        v = pad(v, (p, p, p, p), mode="reflect").reshape(1, B * 3, o + 2 * p, o + 2 * p)
        return conv2d(v, w[k * B * 3:(k + 1) * B * 3], groups=B * 3).reshape(B, 3, o, o)

    def grid(v):
        return torch.round(v.clamp(0, 1) * 255) / 255

    def torch_leg(k):
        arena.crops(desc[sl(k)], gt, s0, deg=deg[sl(k)], ksize=K, jpeg_chroma="420")
        v = conv(s0, wts[0], k)
        z = torch.randn(B, 3, o, o, device="cuda")
        z = torch.where(gray[sl(k)], z[:, :1], z)
        v = grid(v + torch.sqrt(sp[sl(k)] * v.clamp(min=0) + sn[sl(k)] ** 2) * z)
        v = grid(conv(v, wts[1], k))
        v = torch_jpeg(v, q_all[sl(k), 0], q_all[sl(k), 1], on[sl(k)], 1, T)
        lr.copy_(grid(conv(v, wts[2], k)))

    # the comparator is the kernel's model: without noise (the two draw different normals) passes A and B of the two pipelines agree
    # but for pixels whose rounding the summation order decides
    quiet = rows.clone()
    quiet[0, :, 1:3] = 0
    arena.crops(desc[sl(0)], gt, s0, deg=deg[sl(0)], ksize=K, jpeg_chroma="420")
    want = filter2d(filter2d(s0, quiet[0, sl(0)], bank), quiet[1, sl(0)], bank)
    differ = float((((grid(conv(grid(conv(s0, wts[0], 0)), wts[1], 0)) - want).abs() * 255) > 0.5).float().mean())
    assert differ < 0.05, f"the torch pipeline and sst_filter2d differ on {differ:.3f} of the pixels"

    legs = {"off_degraded_jpeg": off}
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        for name in ("sst_gather_crops_degraded", "sst_jpeg"):
            getattr(other, name).restype, getattr(other, name).argtypes = _abi.SIGNATURES[name]
        wy, iy, wx, ix = arena._bicubic.tables_i32(HR, HR, 1.0 / UP, arena.device)

        def parent(k):
            d = deg[sl(k)]
            rc = other.sst_gather_crops_degraded(arena.arena.data_ptr(), arena.arena.numel(), arena.table.data_ptr(), arena.n_images,
                                                 desc[sl(k)].data_ptr(), B, HR, arena.lut.data_ptr(), gt.data_ptr(), lr.data_ptr(),
                                                 wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), o, o, wy.shape[1], wx.shape[1],
                                                 arena.span(True, True), d.data_ptr(), K, 1, _abi.stream_ptr())
            assert rc == 0, rc
            rc = other.sst_jpeg(lr.data_ptr(), d.data_ptr(), B, o, o, 1, _abi.stream_ptr())
            assert rc == 0, rc
        legs["off_degraded_jpeg_parent_lib"] = parent
        if parent_first:                                 # the same two legs in the other order: what the order alone is worth
            legs = {"off_degraded_jpeg_parent_lib": parent, "off_degraded_jpeg": off}
    off(0)
    s0.copy_(lr)
    for j, name in ((0, "pass_a_blur_noise"), (1, "pass_b_sinc_or_through"), (3, "pass_c_sinc_or_through")):
        legs[name] = lambda k, j=j: filter2d(s0, rows[j, sl(k)], bank, out=s1)
    legs["jpeg_2"] = lambda k: jpeg(s1, rows[2, sl(k)], "420", out=s1)
    legs["second_order_batch"] = whole
    legs["torch_ops_batch"] = torch_leg

    graphs = {}
    for name, run in legs.items():
        for k in range(min(3, launches)):               # warm up: tables, code objects, the allocator's pool
            run(k)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for k in range(launches):
                run(k)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    out = {"mode": "second", "batch": B, "hr": HR, "scale": UP, "launches_per_graph": launches, "replays": replays, "repeat": repeat,
           "torch_ops_pixels_off_by_a_level": round(differ, 5),
           "us_per_batch": {name: [] for name in legs}}
    for _ in range(repeat):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                gr.replay()
            t1.record()
            torch.cuda.synchronize()
            out["us_per_batch"][name].append(round(t0.elapsed_time(t1) * 1e3 / (replays * launches), 2))
    out["median_us_per_batch"] = {name: sorted(v)[len(v) // 2] for name, v in out["us_per_batch"].items()}
    print(json.dumps(out))


def resize_mode(launches, replays, repeat, parent_lib, parent_first=False):
    import ctypes
    from srganst import _abi
    from srganst.device_data import (RESIZE_MODES, Degradation, DeviceImageArena, SecondOrder, filter2d, rescale, resize_size,
                                     second_order)
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 2]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    n, K, o = launches * B, 21, HR // UP
    tiles = torch.from_numpy(arena.tiles)[torch.randperm(len(arena), generator=g)[:n]]
    room = torch.from_numpy(arena.table_host[tiles[:, 0].numpy(), 1:3] - HR + 1)
    desc = torch.zeros(n, 4, dtype=torch.int32)
    desc[:, 0] = tiles[:, 0]
    desc[:, 1:3] = (torch.randint(0, 1 << 30, (n, 2), generator=g) % room).to(torch.int32)
    desc[:, 3] = torch.randint(0, 8, (n,), generator=g).to(torch.int32)
    arena.check_desc(desc.numpy())
    desc = desc.cuda()
    deg = Degradation(jpeg_prob=1.0).draw(n, torch.Generator().manual_seed(1)).cuda()
    kw = dict(blur_prob=1.0, noise_prob=1.0, final_sinc_prob=1.0, jpeg_prob=1.0, ksize=K)
    so, so_r = SecondOrder(**kw), SecondOrder(**kw, resize_prob=(0.3, 0.4, 0.3))
    full = so.draw(n, torch.Generator().manual_seed(2))
    rows_off, rows_on = full.cuda(), so_r.draw(n, torch.Generator().manual_seed(2)).cuda()
    bank = torch.from_numpy(so.draw_bank(torch.Generator().manual_seed(3))).cuda()
    drawn_host = so_r.draw_resize(n, o, o, torch.Generator().manual_seed(4), noise=full[0].numpy())
    drawn = drawn_host.cuda()

    def at_scale(s):                                     # every sample at the scale s, the drawn modes (keep: bicubic both ways) and noise
        r = drawn_host.clone()
        r[:, 0] = r[:, 1] = resize_size(o, s)
        keep = drawn_host[:, 0] == 0
        r[keep, 6] |= RESIZE_MODES["bicubic"] | RESIZE_MODES["bicubic"] << 2
        return r.cuda()
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, o, o, device="cuda")
    s0, s1 = torch.empty_like(lr), torch.empty_like(lr)
    sl = lambda k: slice(k * B, (k + 1) * B)

    def off(k):
        arena.crops(desc[sl(k)], gt, s0, deg=deg[sl(k)], ksize=K, jpeg_chroma="420")
        second_order(s0, rows_off[:, sl(k)], bank, "420", out=lr, scratch=(s1, s0))

    def whole(k):
        arena.crops(desc[sl(k)], gt, s0, deg=deg[sl(k)], ksize=K, jpeg_chroma="420")
        second_order(s0, rows_on[:, sl(k)], bank, "420", out=lr, scratch=(s1, s0), resize_rows=drawn[sl(k)])

    # ---- the comparator for R alone: the drawn round trips as torch ops, one F.interpolate pair per sample (the sizes differ per
    # sample, so the batch cannot be one call), noise at the intermediate size, clamp, round
    interp = torch.nn.functional.interpolate
    names = {v: k for k, v in RESIZE_MODES.items()}
    sn, sp = (drawn[:, j].contiguous().view(torch.float32) for j in (2, 3))
    plan = [(int(r[0]), int(r[1]), names[int(r[6]) & 3], names[(int(r[6]) >> 2) & 3], bool(int(r[6]) >> 4 & 1)) for r in drawn_host.tolist()]

    def torch_leg(k):
        for b in range(B):
            i = k * B + b
            hi, wi, m1, m2, gray = plan[i]
            v = s0[b:b + 1]
            if hi:
                v = interp(v, size=(hi, wi), mode=m1, **({} if m1 == "area" else {"align_corners": False}))
            z = torch.randn(1, 1 if gray else 3, v.shape[2], v.shape[3], device="cuda")
            v = v + torch.sqrt(sp[i] * v.clamp(min=0) + sn[i] ** 2) * z
            if hi:
                v = interp(v, size=(o, o), mode=m2, **({} if m2 == "area" else {"align_corners": False}))
            s1[b:b + 1] = torch.round(v.clamp(0, 1) * 255) / 255

    # the comparator is the kernel's model: without noise the two agree but for pixels whose rounding the summation order decides
    off(0)
    s0.copy_(lr)
    quiet = drawn[sl(0)].clone()
    quiet[:, 2:4] = 0
    want = rescale(s0, quiet)
    sn_keep, sp_keep = sn.clone(), sp.clone()
    sn.zero_(), sp.zero_()
    torch_leg(0)
    sn.copy_(sn_keep), sp.copy_(sp_keep)
    differ = float((((s1 - want).abs() * 255) > 0.5).float().mean())
    assert differ < 0.05, f"the torch round trip and sst_rescale differ on {differ:.3f} of the pixels"

    legs = {"off_second_order_batch": off}
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        for name in ("sst_gather_crops_degraded", "sst_jpeg", "sst_filter2d"):
            getattr(other, name).restype, getattr(other, name).argtypes = _abi.SIGNATURES[name]
        wy, iy, wx, ix = arena._bicubic.tables_i32(HR, HR, 1.0 / UP, arena.device)
        M = bank.shape[0]

        def parent(k):
            d, st = deg[sl(k)], _abi.stream_ptr()
            rcs = [other.sst_gather_crops_degraded(arena.arena.data_ptr(), arena.arena.numel(), arena.table.data_ptr(), arena.n_images,
                                                   desc[sl(k)].data_ptr(), B, HR, arena.lut.data_ptr(), gt.data_ptr(), s0.data_ptr(),
                                                   wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), o, o, wy.shape[1],
                                                   wx.shape[1], arena.span(True, True), d.data_ptr(), K, 1, st),
                   other.sst_jpeg(s0.data_ptr(), d.data_ptr(), B, o, o, 1, st)]
            r = rows_off[:, sl(k)]
            rcs.append(other.sst_filter2d(s0.data_ptr(), s1.data_ptr(), r[0].data_ptr(), bank.data_ptr(), M, B, o, o, K, 1, st))
            rcs.append(other.sst_filter2d(s1.data_ptr(), s0.data_ptr(), r[1].data_ptr(), bank.data_ptr(), M, B, o, o, K, 1, st))
            rcs.append(other.sst_jpeg(s0.data_ptr(), r[2].data_ptr(), B, o, o, 1, st))
            rcs.append(other.sst_filter2d(s0.data_ptr(), lr.data_ptr(), r[3].data_ptr(), bank.data_ptr(), M, B, o, o, K, 1, st))
            assert not any(rcs), rcs
        legs["off_second_order_batch_parent_lib"] = parent
        if parent_first:                                 # the same two legs in the other order: what the order alone is worth
            legs = {"off_second_order_batch_parent_lib": parent, "off_second_order_batch": off}
    off(0)
    s0.copy_(lr)
    for s in (0.3, 1.0, 1.2):
        legs[f"rescale_alone_s{s:g}"] = lambda k, r=at_scale(s): rescale(s0, r[sl(k)], out=s1)
    legs["rescale_alone_drawn"] = lambda k: rescale(s0, drawn[sl(k)], out=s1)
    legs["pass_a_blur_unquantised"] = lambda k: filter2d(s0, rows_on[0, sl(k)], bank, quantise=False, out=s1)
    legs["torch_ops_rescale_alone_drawn"] = torch_leg
    legs["second_order_batch_with_resize"] = whole

    graphs = {}
    for name, run in legs.items():
        for k in range(min(3, launches)):               # warm up: tables, code objects, the allocator's pool
            run(k)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for k in range(launches):
                run(k)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    out = {"mode": "resize", "batch": B, "hr": HR, "scale": UP, "launches_per_graph": launches, "replays": replays, "repeat": repeat,
           "torch_ops_pixels_off_by_a_level": round(differ, 5),
           "us_per_batch": {name: [] for name in legs}}
    for _ in range(repeat):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                gr.replay()
            t1.record()
            torch.cuda.synchronize()
            out["us_per_batch"][name].append(round(t0.elapsed_time(t1) * 1e3 / (replays * launches), 2))
    out["median_us_per_batch"] = {name: sorted(v)[len(v) // 2] for name, v in out["us_per_batch"].items()}
    print(json.dumps(out))


def resize1_mode(launches, replays, repeat, parent_lib, parent_first=False):
    import ctypes
    from srganst import _abi
    from srganst.device_data import RESIZE_MODES, Degradation, DeviceImageArena, blur, rescale_to, resize1_size
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in WHOLE_SIZES * 2]
    arena = DeviceImageArena.from_arrays(imgs, HR, HR, UP, "cuda")
    n, K, o = launches * B, 21, HR // UP
    tiles = torch.from_numpy(arena.tiles)[torch.randperm(len(arena), generator=g)[:n]]
    room = torch.from_numpy(arena.table_host[tiles[:, 0].numpy(), 1:3] - HR + 1)
    desc = torch.zeros(n, 4, dtype=torch.int32)
    desc[:, 0] = tiles[:, 0]
    desc[:, 1:3] = (torch.randint(0, 1 << 30, (n, 2), generator=g) % room).to(torch.int32)
    desc[:, 3] = torch.randint(0, 8, (n,), generator=g).to(torch.int32)
    arena.check_desc(desc.numpy())
    desc = desc.cuda()
    first = Degradation(resize_prob=(0.2, 0.7, 0.1))
    deg_host = first.draw(n, torch.Generator().manual_seed(1))
    drawn_host = first.draw_resize(n, HR, HR, torch.Generator().manual_seed(5), deg_rows=deg_host.numpy())
    deg, drawn = deg_host.cuda(), drawn_host.cuda()

    def at_scale(s):                                     # every sample at the scale s, the drawn modes (keep: bicubic there) and noise
        r = drawn_host.clone()
        r[:, 0] = r[:, 1] = resize1_size(HR, s)
        r[drawn_host[:, 0] == 0, 6] |= RESIZE_MODES["bicubic"]
        return r.cuda()
    gt, lr = torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, o, o, device="cuda")
    hr = torch.empty_like(gt)
    sl = lambda k: slice(k * B, (k + 1) * B)

    def off(k):
        arena.crops(desc[sl(k)], gt, lr, deg=deg[sl(k)], ksize=K)

    def whole(k):
        arena.crops(desc[sl(k)], gt, with_lr=False)
        rescale_to(blur(gt, deg[sl(k)], K, out=hr), drawn[sl(k)], (o, o), out=lr)

    # ---- the comparator: the same first stage as torch ops behind the plain gather - reflect pad and a grouped conv2d with the
    # per-sample weights (made beforehand), then one F.interpolate pair PER SAMPLE (the intermediate sizes differ per sample), randn
    # noise between them, clamp, round
    interp, pad, conv2d = torch.nn.functional.interpolate, torch.nn.functional.pad, torch.nn.functional.conv2d
    names = {v: k for k, v in RESIZE_MODES.items()}
    sn = drawn[:, 2].contiguous().view(torch.float32)
    plan = [(int(r[0]), int(r[1]), names[int(r[6]) & 3], names[(int(r[6]) >> 2) & 3]) for r in drawn_host.tolist()]
    q = deg[:, :3].contiguous().view(torch.float32).double()
    d = torch.arange(-(K // 2), K // 2 + 1, device="cuda", dtype=torch.float64)
    dy, dx = d[None, :, None], d[None, None, :]
    wts = torch.exp(-(q[:, 0, None, None] * dx * dx + q[:, 1, None, None] * dx * dy + q[:, 2, None, None] * dy * dy))
    wts = (wts / wts.sum((1, 2), keepdim=True)).float()
    ident = torch.zeros(K, K, device="cuda")
    ident[K // 2, K // 2] = 1.0
    wts[q[:, 0] < 0] = ident                             # the no-blur sentinel: the identity kernel, the same ops for every sample
    wts = wts.repeat_interleave(3, 0)[:, None].contiguous()
    p = K // 2
    mode_kw = lambda m: {} if m == "area" else {"align_corners": False}

    def torch_resize(k, src):
        for b in range(B):
            i = k * B + b
            hi, wi, m1, m2 = plan[i]
            v = src[b:b + 1]
            if hi:
                v = interp(v, size=(hi, wi), mode=m1, **mode_kw(m1))
            v = v + sn[i] * torch.randn(1, 3, v.shape[2], v.shape[3], device="cuda")
            v = interp(v, size=(o, o), mode=m2, **mode_kw(m2))
            lr[b:b + 1] = torch.round(v.clamp(0, 1) * 255) / 255

    def torch_leg(k):
        arena.crops(desc[sl(k)], gt, with_lr=False)
        x = pad(gt, (p, p, p, p), mode="reflect").reshape(1, B * 3, HR + 2 * p, HR + 2 * p)
        torch_resize(k, conv2d(x, wts[k * B * 3:(k + 1) * B * 3], groups=B * 3).reshape(B, 3, HR, HR))

    # the comparator is the kernel's model: without noise the two agree but for pixels whose rounding the summation order decides
    arena.crops(desc[sl(0)], gt, with_lr=False)
    blur(gt, deg[sl(0)], K, out=hr)
    quiet = drawn[sl(0)].clone()
    quiet[:, 2] = 0
    want = rescale_to(hr, quiet, (o, o))
    sn_keep = sn.clone()
    sn.zero_()
    torch_resize(0, hr)
    sn.copy_(sn_keep)
    differ = float((((lr - want).abs() * 255) > 0.5).float().mean())
    assert differ < 0.05, f"the torch resize pair and sst_rescale_to differ on {differ:.3f} of the pixels"

    legs = {"off_degraded_gather_k21": off}
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        other.sst_gather_crops_degraded.restype, other.sst_gather_crops_degraded.argtypes = _abi.SIGNATURES["sst_gather_crops_degraded"]
        wy, iy, wx, ix = arena._bicubic.tables_i32(HR, HR, 1.0 / UP, arena.device)

        def parent(k):
            rc = other.sst_gather_crops_degraded(arena.arena.data_ptr(), arena.arena.numel(), arena.table.data_ptr(), arena.n_images,
                                                 desc[sl(k)].data_ptr(), B, HR, arena.lut.data_ptr(), gt.data_ptr(), lr.data_ptr(),
                                                 wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), o, o, wy.shape[1], wx.shape[1],
                                                 arena.span(True, True), deg[sl(k)].data_ptr(), K, 1, _abi.stream_ptr())
            assert rc == 0, rc
        legs["off_degraded_gather_k21_parent_lib"] = parent
        if parent_first:                                 # the same two legs in the other order: what the order alone is worth
            legs = {"off_degraded_gather_k21_parent_lib": parent, "off_degraded_gather_k21": off}
    legs["plain_gather_gt_alone"] = lambda k: arena.crops(desc[sl(k)], gt, with_lr=False)
    legs["blur_alone"] = lambda k: blur(gt, deg[sl(k)], K, out=hr)
    for s in (0.15, 1.0, 1.5):
        legs[f"rescale_to_alone_s{s:g}"] = lambda k, r=at_scale(s): rescale_to(hr, r[sl(k)], (o, o), out=lr)
    legs["rescale_to_alone_drawn"] = lambda k: rescale_to(hr, drawn[sl(k)], (o, o), out=lr)
    legs["first_stage_three_launches"] = whole
    legs["torch_ops_first_stage"] = torch_leg

    graphs = {}
    for name, run in legs.items():
        for k in range(min(3, launches)):               # warm up: tables, code objects, the allocator's pool
            run(k)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for k in range(launches):
                run(k)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    out = {"mode": "resize1", "batch": B, "hr": HR, "scale": UP, "launches_per_graph": launches, "replays": replays, "repeat": repeat,
           "torch_ops_pixels_off_by_a_level": round(differ, 5),
           "us_per_batch": {name: [] for name in legs}}
    for _ in range(repeat):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                gr.replay()
            t1.record()
            torch.cuda.synchronize()
            out["us_per_batch"][name].append(round(t0.elapsed_time(t1) * 1e3 / (replays * launches), 2))
    out["median_us_per_batch"] = {name: sorted(v)[len(v) // 2] for name, v in out["us_per_batch"].items()}
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("second", "resize", "resize1"):
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--launches", type=int, default=32)
        ap.add_argument("--replays", type=int, default=50)
        ap.add_argument("--repeat", type=int, default=5)
        ap.add_argument("--parent-lib", default="", help="another build of libsrganst.so whose off path is timed beside this one's")
        ap.add_argument("--parent-first", action="store_true", help="time the parent library's leg before this library's")
        a = ap.parse_args()
        mode = {"second": second_mode, "resize": resize_mode, "resize1": resize1_mode}[a.mode]
        return mode(a.launches, a.replays, a.repeat, a.parent_lib, a.parent_first)
    if len(sys.argv) > 1 and sys.argv[1] == "jpeg":
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--launches", type=int, default=32)
        ap.add_argument("--replays", type=int, default=50)
        ap.add_argument("--repeat", type=int, default=5)
        ap.add_argument("--parent-lib", default="", help="another build of libsrganst.so whose degraded gather is timed beside this one's")
        ap.add_argument("--parent-first", action="store_true", help="time the parent library's leg before this library's")
        a = ap.parse_args()
        return jpeg_mode(a.launches, a.replays, a.repeat, a.parent_lib, a.parent_first)
    if len(sys.argv) > 1 and sys.argv[1] == "degrade":
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--launches", type=int, default=32)
        ap.add_argument("--replays", type=int, default=50)
        ap.add_argument("--repeat", type=int, default=5)
        ap.add_argument("--parent-lib", default="", help="another build of libsrganst.so whose sst_gather_crops is timed beside this one's")
        a = ap.parse_args()
        return degrade_mode(a.launches, a.replays, a.repeat, a.parent_lib)
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--skip", type=int, default=20)
    ap.add_argument("--cases", default="device,host,host_lr,on_device")
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--crops", default="", help="with --gather-only: grid, odd_x0 or transposed (sst_gather_crops beside sst_gather_batch)")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    if a.gather_only:
        return gather_crops_only(a.iters, a.crops) if a.crops else gather_only(a.iters)
    if a.images < (a.skip + a.steps + 1) * B:
        raise SystemExit(f"--images {a.images} < {(a.skip + a.steps + 1) * B}: the timed window must fit into one epoch")
    cases = a.cases.split(",")
    out = {"batch": B, "hr": HR, "images": a.images, "steps": a.steps, "skip": a.skip}
    with tempfile.TemporaryDirectory() as tmp:
        gt_dir = os.path.join(tmp, "train")
        os.makedirs(gt_dir)
        t0 = time.perf_counter()
        write_crops(gt_dir, a.images)
        out["png_write_s"] = round(time.perf_counter() - t0, 2)
        os.chdir(tmp)                                   # train() writes results/<name>/ checkpoints under the working directory
        if "on_device" in cases:
            from srganst.device_data import DeviceImageSet, decode_threads
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = DeviceImageSet.from_dir(gt_dir, UP, "cuda")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["decode_upload_s"] = round(dt, 3)
            out["decode_upload_img_s"] = round(len(s) / dt, 1)
            out["decode_threads"] = decode_threads()
            out["store_bytes"] = s.store.numel()
            del s
        whole_dir = os.path.join(tmp, "original")
        if any(c.startswith("whole_images") for c in cases):
            from srganst.device_data import DeviceImageArena, decode_threads
            os.makedirs(whole_dir)
            t0 = time.perf_counter()
            out["whole_images"] = write_whole_images(whole_dir, a.images)
            out["whole_png_write_s"] = round(time.perf_counter() - t0, 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = DeviceImageArena.from_dir(whole_dir, HR, HR, UP, "cuda")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["whole_decode_upload_s"] = round(dt, 3)
            out["whole_decode_threads"] = decode_threads()
            out["whole_arena_bytes"] = s.arena.numel()
            out["whole_tiles"] = len(s)
            del s
        whole = {"DATA.ON_DEVICE_WHOLE_IMAGES": True, "DATA.TRAIN_ORIGINAL_IMAGES_DIR": whole_dir, "DATA.CROP_STEP": HR}
        runs = {
            "device": lambda: time_device_tensors(gt_dir, a.skip, a.steps),
            "host": lambda: time_train(gt_dir, "tl_host", a.skip, a.steps),
            "host_lr": lambda: time_train(gt_dir, "tl_host_lr", a.skip, a.steps, **{"KERNEL.LR_ON_DEVICE": True}),
            "on_device": lambda: time_train(gt_dir, "tl_on_device", a.skip, a.steps, **{"DATA.ON_DEVICE": True}),
            "whole_images": lambda: time_train(gt_dir, "tl_whole", a.skip, a.steps, **whole),
            "whole_images_aug": lambda: time_train(gt_dir, "tl_whole_aug", a.skip, a.steps, **whole,
                                                   **{"DATA.RANDOM_CROP": True, "DATA.AUGMENT": True}),
        }
        for rep in range(a.repeat):
            for c in cases:
                sec = runs[c]()
                out[f"{c}_ms_per_step"] = round(sec * 1e3, 3)           # (the last repeat's)
                out[f"{c}_img_s"] = round(B / sec, 1)
                out.setdefault(f"{c}_ms_per_step_repeats", []).append(round(sec * 1e3, 3))
                print(f"# {c} [{rep + 1}/{a.repeat}]: {sec * 1e3:.3f} ms/step, {B / sec:.1f} img/s", file=sys.stderr, flush=True)
        if "device" in cases and "on_device" in cases:
            out["on_device_vs_device_tensors"] = round(out["device_ms_per_step"] / out["on_device_ms_per_step"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
