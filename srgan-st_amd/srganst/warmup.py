"""SRResNet pre-training driver.  Mirrors reference warmup.py:14-147: seed, Generator, Adam(eps 1e-4),
loaders, per-epoch step loop, validation, checkpoints (g_last / g_best / g_epochN with the reference's
state-dict keys).  The step itself is srganst.engine.WarmupEngine (HIP kernels, hipGraph, RCCL).
EXP.RESUME / SOLVER.G_EMA_DECAY: as in train.py (training state and averaged generator, checkpoint.py)."""
from __future__ import annotations

import os

import torch
from torch.utils.data import DataLoader

from . import checkpoint
from . import device_data
from . import dist as sdist
from .bicubic import Bicubic
from .config import Config
from .dataset import TestImageDataset, TrainImageDataset
from .engine import WarmupEngine
from .model import Generator
from .utils import init_random_seed, start_workers
from .validate import _validate


class _NullWriter:
    def add_scalar(self, *a, **k): pass
    def add_text(self, *a, **k): pass


def _writer(name):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(f"tensorboard/{name}")
    except Exception:
        return _NullWriter()


def log_grad_stats(writer, stats, batches_done):
    """Train/{G,D}_GradNorm, _ClipCoef, _Skipped for the networks whose optimizer clips or guards (engine.grad_stats()); returns
    the skipped counts as a piece of the printed line ("" with the feature off)."""
    line = ""
    for net, st in stats.items():
        if st is None:
            continue
        writer.add_scalar(f"Train/{net}_GradNorm", st["norm"], batches_done)
        writer.add_scalar(f"Train/{net}_ClipCoef", st["coef"], batches_done)
        writer.add_scalar(f"Train/{net}_Skipped", st["n_skipped"], batches_done)
        line += f" [{net} skipped: {st['n_skipped']}/{st['n_steps_seen']}]"
    return line


def warmup(config: Config, train_dataset=None, test_dataset=None, max_steps_per_epoch=None):
    rank, local, world = sdist.init_from_env(config.DIST.BACKEND)
    init_random_seed(config.DATA.SEED)
    best_psnr = best_ssim = 0.0
    batches_done = 0
    # EXP.RESUME: START_EPOCH comes from the file BEFORE the loaders are built (the on-device loaders key their draws on it)
    resume = checkpoint.load_resume(config, world)
    if resume is not None:
        best_psnr, best_ssim, batches_done = resume["best_psnr"], resume["best_ssim"], resume["batches_done"]
    generator = Generator(config).to(config.DEVICE)
    if resume is not None:                       # before the engine is built: its flat parameter buffer sees the weights
        generator.load_state_dict(resume["generator"])
    sdist.broadcast_module(generator)
    engine = WarmupEngine(config, generator)
    if resume is not None:
        engine.opt.load_state_dict(resume["g_opt"])
        if engine.g_ema is not None:
            engine.g_ema.load_state_dict(resume["g_ema"])
        engine.load_clip_state(resume.get("clip"))       # absent (written with the feature off): the counters start at zero
    ema_validate = engine.g_ema is not None and bool(config.SOLVER.get("G_EMA_VALIDATE", True))
    train_ds = train_dataset or TrainImageDataset(config.DATA.TRAIN_GT_IMAGES_DIR, config.DATA.UPSCALE_FACTOR)
    test_ds = test_dataset or TestImageDataset(config.DATA.TEST_GT_IMAGES_DIR, config.DATA.TEST_LR_IMAGES_DIR)
    on_device = device_data.on_device(config)    # DATA.ON_DEVICE or DATA.ON_DEVICE_WHOLE_IMAGES
    if on_device:                                # HBM-resident set, one gather launch per batch (device_data.py)
        train_loader, sampler = device_data.train_loader(config, train_dataset, world, rank)
    else:
        sampler = torch.utils.data.distributed.DistributedSampler(train_ds, world, rank, shuffle=True) if world > 1 else None
        train_loader = DataLoader(train_ds, batch_size=config.DATA.BATCH_SIZE, shuffle=sampler is None, sampler=sampler,
                                  num_workers=1, pin_memory=True, drop_last=True, persistent_workers=True)
    test_loader = DataLoader(test_ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    if config.DATA.VALIDATE_ON_DEVICE and rank == 0:       # the validation pairs on the device, once (only rank 0 validates)
        test_loader = device_data.DeviceTestSet.from_dataset(test_ds, config.DEVICE)
    device_bicubic = Bicubic(config.DEVICE)
    start_workers(train_loader)                  # fork the loader workers with the collector frozen (see utils.start_workers)
    writer = _writer(config.EXP.NAME) if rank == 0 else _NullWriter()
    writer.add_text("Config/Params", config.get_all_params())
    if resume is not None:      # last: model construction and start_workers have drawn from the streams by now
        checkpoint.restore_rng(resume["rng"], config.DEVICE)
    resume = None
    for epoch in range(config.EXP.START_EPOCH, config.EXP.N_EPOCHS):
        if rank == 0:
            print(f"Beginning warmup epoch: {epoch+1}")
        generator.train()
        if sampler is not None:
            sampler.set_epoch(epoch)
        for batch_num, (gt, lr) in enumerate(train_loader):
            if max_steps_per_epoch is not None and batch_num >= max_steps_per_epoch:
                break
            batches_done += 1
            if not on_device:                        # (on device: the batch is made in the engine's input buffers once bound)
                # host batch straight into the engine's static input buffers when they exist and fit (copy_ returns the buffer)
                fits = engine.gt is not None and engine.gt.shape == gt.shape
                gt = engine.gt.copy_(gt, non_blocking=True) if fits else gt.to(device=config.DEVICE, non_blocking=True)
                if config.KERNEL.LR_ON_DEVICE:
                    lr = device_bicubic(gt, scale=1.0 / config.DATA.UPSCALE_FACTOR)
                elif fits and engine.lr.shape == lr.shape:
                    lr = engine.lr.copy_(lr, non_blocking=True)
                else:
                    lr = lr.to(device=config.DEVICE, non_blocking=True)
            loss_values = engine.step(gt, lr)
            if on_device:
                train_loader.bind(engine.gt, engine.lr)
            if batch_num % config.LOG_TRAIN_PERIOD != 0 or rank != 0:
                continue
            vals = {k: float(v) for k, v in loss_values.items()}          # the only host sync, on log steps
            writer.add_scalar("Train/G_Loss", sum(vals.values()), batches_done)
            for name, v in vals.items():
                writer.add_scalar(f"Train/G_{name}", v, batches_done)
            skipped = log_grad_stats(writer, engine.grad_stats(), batches_done)
            print(f"[Epoch {epoch+1}/{config.EXP.N_EPOCHS}] [Batch {batch_num}/{len(train_loader)}] [G losses: {vals}]{skipped}")
        generator.eval()
        if rank == 0:
            engine.sync_ema_buffers()             # the averaged generator takes G's BatchNorm buffers before it is run or saved
            # (psnr, ssim) + (st,) with DATA.VALIDATE_ST + (lr_psnr,) with DATA.VALIDATE_LR; with the average on (and G_EMA_VALIDATE)
            # it is the averaged generator's
            psnr, ssim, *more = _validate(engine.g_ema if ema_validate else generator, test_loader, config)
            st = more[:1] if config.DATA.get("VALIDATE_ST", False) else []
            lr_psnr = more[-1:] if config.DATA.get("VALIDATE_LR", False) else []
            if epoch % config.LOG_VALIDATION_PERIOD == 0:
                print(f"[Test: {epoch+1}/{config.EXP.N_EPOCHS}] [PSNR: {psnr}] [SSIM: {ssim}]")
            writer.add_scalar("Test/PSNR", psnr, epoch + 1)
            writer.add_scalar("Test/SSIM", ssim, epoch + 1)
            if st:
                writer.add_scalar("Test/ST", st[0], epoch + 1)
            if lr_psnr:
                writer.add_scalar("Test/LR-PSNR", lr_psnr[0], epoch + 1)
            results_dir = f"results/{config.EXP.NAME}"
            os.makedirs(results_dir, exist_ok=True)
            torch.save(generator.state_dict(), results_dir + "/g_last.pth")
            if engine.g_ema is not None:
                torch.save(engine.g_ema.state_dict(), results_dir + "/g_ema_last.pth")
            if best_psnr < psnr and best_ssim < ssim:
                torch.save(generator.state_dict(), results_dir + "/g_best.pth")
                if engine.g_ema is not None:
                    torch.save(engine.g_ema.state_dict(), results_dir + "/g_ema_best.pth")
                best_psnr, best_ssim = psnr, ssim
            if 0 < epoch and epoch % config.G_CHECKPOINT_INTERVAL == 0:
                torch.save(generator.state_dict(), results_dir + f"/g_epoch{epoch}.pth")
                if engine.g_ema is not None:
                    torch.save(engine.g_ema.state_dict(), results_dir + f"/g_ema_epoch{epoch}.pth")
            if config.EXP.get("SAVE_STATE", True):       # last in the epoch: the RNG streams go in as the next epoch will find them
                checkpoint.save_training_state(results_dir + "/" + checkpoint.STATE_FILE, epoch=epoch + 1, generator=generator,
                                               g_opt=engine.opt, g_sched=None, g_ema=engine.g_ema, best=(best_psnr, best_ssim),
                                               batches_done=batches_done, config=config, world_size=world,
                                               clip=engine.clip_state())
    engine.close()
    return generator


if __name__ == "__main__":
    warmup(Config())
