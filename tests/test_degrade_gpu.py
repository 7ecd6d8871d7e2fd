"""GPU: the blind-SR degradation stage (csrc/degrade.h: sst_gather_crops_degraded, sst_degrade; srganst.device_data: Degradation,
degrade, DeviceImageArena.crops(deg=...), DeviceCropLoader(degradation=...)) against the fp64 restatement of tests/degrade_refs.py:
identity samples, the unquantised and the quantised values, the two entries' bit equality, the general entry's tiling, the noise's
determinism, a captured launch, the loader and the drivers.

Two cases of the issue cannot be run as it words them and are run like this instead: a 32-px crop fits none of the three images of
the small arena, so that case alone adds a fourth image (degrade_refs.ARENA_SIZES_32); and K = 21 (p = 10) is refused for the 9 x 11
image (p >= 9, itself one of the refusals to test), which is degraded with K = 17 and K = 7 instead."""
import math
import os
import re

import numpy as np
import pytest
import torch

import degrade_refs as refs
from test_degrade_refs import CROP_CASES, KERNELS

pytestmark = pytest.mark.gpu

BOUND = refs.BOUND       # max abs error of the unquantised values: (K^2 + Ty + Tx + 4) * 2^-24 * sum|w| * max|x| at K = 21


def _arena(S, scale):
    from srganst.device_data import DeviceImageArena
    imgs = refs.arena_images(S)
    arena = DeviceImageArena.from_arrays(imgs, S, 8, scale, "cuda")
    batch = refs.arena_descriptors(imgs, S)
    assert sorted(d[3] for d in batch) == list(range(8))
    arena.check_desc(batch)
    return imgs, arena, batch, torch.tensor(batch, dtype=torch.int32, device="cuda")


def _rows(s1, s2, th, noise, n, ksize, key0=100):
    """n rows with these parameters and keys key0, key0 + 1, .."""
    from srganst.device_data import Degradation
    return torch.cat([Degradation.fixed(s1, s2, th, noise, key0 + i, ksize=ksize).draw(1) for i in range(n)])


def _mixed_rows(n, ksize, noise=True):
    """n rows that differ in every parameter: the three kernels and the sentinel in turn, noise on every other row."""
    ks = KERNELS + [(0.0, 0.0, 0.0)]
    return torch.cat([_rows(*ks[i % 4], 25.0 if noise and i % 2 else 0.0, 1, ksize, key0=7 + 13 * i) for i in range(n)])


@pytest.mark.parametrize("S, scale, K", [(24, 4, 21), (8, 2, 7)])
def test_identity_sample_takes_the_plain_gathers_bits(S, scale, K):
    _, arena, batch, desc = _arena(S, scale)
    gt0, lr0 = arena.crops(desc)
    deg = _rows(0, 0, 0, 0.0, len(batch), K).cuda()
    gt1, lr1 = arena.crops(desc, deg=deg, ksize=K)
    assert torch.equal(gt0, gt1) and torch.equal(lr0, lr1)
    none, lr2 = arena.crops(desc, deg=deg, ksize=K, with_gt=False)
    assert none is None and torch.equal(lr0, lr2)
    # unquantised: the bicubic sums themselves, which round to the plain launch's values
    _, raw = arena.crops(desc, deg=deg, ksize=K, quantise=False)
    assert torch.equal(torch.round(255 * raw), torch.round(255 * lr0)) and not torch.equal(raw, lr0)


@pytest.mark.parametrize("kernel", range(len(KERNELS)))
@pytest.mark.parametrize("S, scale, K", CROP_CASES)
def test_crops_against_the_fp64_restatement(S, scale, K, kernel):
    """Unquantised: max abs error <= 3e-5, the a-priori bound; quantised: the reference's rounding, or one grid step from it where
    the reference alone calls the rounding ambiguous - under 1 % of the pixels; gt: the plain launch's."""
    from srganst.device_data import crops_reference
    imgs, arena, batch, desc = _arena(S, scale)
    gt_ref, _ = crops_reference(imgs, batch, S, scale)
    assert S // scale >= 1 and K // 2 < S
    for noise in (0.0, 25.0):
        deg = _rows(*KERNELS[kernel], noise, len(batch), K)
        ref = refs.degrade_reference(gt_ref.numpy(), deg.numpy(), scale, K, quantise=False)
        gt, raw = arena.crops(desc, deg=deg.cuda(), ksize=K, quantise=False)
        assert torch.equal(gt.cpu(), gt_ref) and tuple(raw.shape) == (len(batch), 3, S // scale, S // scale)
        err = float(np.abs(raw.cpu().double().numpy() - ref).max())
        print(f"[degrade S {S} x{scale} K {K} kernel {KERNELS[kernel]} noise {noise:g}] max abs error {err:.3e} (bound {BOUND:.0e})")
        assert err <= BOUND, err
        gt, lr = arena.crops(desc, deg=deg.cuda(), ksize=K)
        differ = refs.check_quantised(lr.cpu().numpy(), ref, deg.numpy(), f"S {S} x{scale} K {K} kernel {kernel} noise {noise:g}")
        assert differ < 0.01 * lr.numel() and torch.equal(gt.cpu(), gt_ref)
        if noise:
            assert float(lr.min()) >= 0 and float(lr.max()) <= 1


@pytest.mark.parametrize("S, scale, K", [(24, 4, 21), (24, 4, 5), (32, 8, 9), (8, 2, 7), (12, 4, 21)])
def test_both_entries_run_one_code_path(S, scale, K):
    """crops(desc, deg)'s lr equals degrade(its gt, deg) bit for bit: all eight transforms, every kernel and the sentinel, with and
    without noise, quantised and not."""
    from srganst.device_data import degrade
    _, arena, batch, desc = _arena(S, scale)
    for noise in (False, True):
        deg = _mixed_rows(len(batch), K, noise).cuda()
        for quantise in (True, False):
            gt, lr = arena.crops(desc, deg=deg, ksize=K, quantise=quantise)
            assert torch.equal(lr, degrade(gt, deg, scale, K, quantise)), (noise, quantise)
            assert bool(torch.isfinite(lr).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H, W, scale, K", [(23, 30, 4, 21), (9, 11, 2, 17), (9, 11, 2, 7), (12, 12, 4, 21), (13, None, 4, 21), (40, None, 8, 9)])
def test_general_entry(H, W, scale, K, B):
    """Any H, W: not multiples of the scale, not equal, smaller than the window, and one LR pixel wider than the column tile (W =
    None: the width from the tile constant that device_data exports); different parameters per sample."""
    from srganst import device_data
    if W is None:
        W = (device_data.DEGRADE_TILE_COLS + 1) * scale + 1
        assert W // scale == device_data.DEGRADE_TILE_COLS + 1
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255
    for noise in (False, True):
        deg = _rows(*KERNELS[2], 25.0 if noise else 0.0, 1, K) if B == 1 else _mixed_rows(B, K, noise)   # B = 1: the anisotropic kernel
        ref = refs.degrade_reference(x.numpy(), deg.numpy(), scale, K, quantise=False)
        raw = device_data.degrade(x.cuda(), deg.cuda(), scale, K, quantise=False)
        assert tuple(raw.shape) == (B, 3, H // scale, W // scale)
        err = float(np.abs(raw.cpu().double().numpy() - ref).max())
        print(f"[degrade general {H}x{W} x{scale} K {K} B {B} noise {noise}] max abs error {err:.3e} (bound {BOUND:.0e})")
        assert err <= BOUND, err
        lr = device_data.degrade(x.cuda(), deg.cuda(), scale, K)
        differ = refs.check_quantised(lr.cpu().numpy(), ref, deg.numpy(), f"general {H}x{W} x{scale} K {K} B {B}")
        assert differ <= max(1, 0.01 * lr.numel())


def test_general_entry_refuses_a_window_wider_than_the_image():
    from srganst import _abi, device_data
    deg = _rows(1.0, 1.0, 0, 0, 1, 21).cuda()
    for H, W in ((9, 11), (30, 10), (10, 10)):
        with pytest.raises(_abi.HipPathError, match="half window 10"):
            device_data.degrade(torch.zeros(1, 3, H, W, device="cuda"), deg, 2, 21)
    assert tuple(device_data.degrade(torch.zeros(1, 3, 11, 11, device="cuda"), deg, 2, 21).shape) == (1, 3, 5, 5)


def test_noise_is_a_function_of_the_sample_alone():
    from srganst.device_data import degrade
    S, scale, K = 24, 4, 21
    _, arena, batch, desc = _arena(S, scale)
    B = len(batch)
    deg = _mixed_rows(B, K).cuda()
    deg[:, 3] = torch.tensor(25 / 255, dtype=torch.float32).view(torch.int32)           # noise on every row
    gt, a = arena.crops(desc, deg=deg, ksize=K, quantise=False)
    _, b = arena.crops(desc, deg=deg, ksize=K, quantise=False)
    assert torch.equal(a, b)                                                            # same inputs, same bits
    other = deg.clone()
    other[:, 4] += 1
    _, c = arena.crops(desc, deg=other, ksize=K, quantise=False)
    assert all(not torch.equal(a[i], c[i]) for i in range(B))                           # another key, another field
    z = (c - a)[0].flatten().cpu().double() * 255 / 25                                  # z' - z of two independent fields
    assert abs(float(z.mean())) < 0.5 and 0.9 < float(z.std()) < 2.0
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device="cuda")[:B]
    _, d = arena.crops(desc[perm].contiguous(), deg=deg[perm].contiguous(), ksize=K, quantise=False)
    assert torch.equal(d, a[perm])                                                      # a sample sees neither its position nor B
    _, e = arena.crops(desc[2:3].contiguous(), deg=deg[2:3].contiguous(), ksize=K, quantise=False)
    assert torch.equal(e[0], a[2])
    assert torch.equal(degrade(gt[perm].contiguous(), deg[perm].contiguous(), scale, K, False), a[perm])
    # sigma_n = 0 with blur: exactly the noise-free bits, whatever the key
    quiet, quiet2 = deg.clone(), other.clone()
    quiet[:, 3] = quiet2[:, 3] = 0
    _, f = arena.crops(desc, deg=quiet, ksize=K, quantise=False)
    _, h = arena.crops(desc, deg=quiet2, ksize=K, quantise=False)
    assert torch.equal(f, h) and not torch.equal(f, a)
    blurred = [i for i in range(B) if i % 4 != 3]
    ref = refs.degrade_reference(gt.cpu().numpy(), quiet.cpu().numpy(), scale, K, quantise=False)
    assert float(np.abs(f.cpu().double().numpy() - ref)[blurred].max()) <= BOUND
    # weights that do not sum to a finite positive number: a NaN LR for that sample only, gt untouched
    bad = deg.clone()
    bad[1, 0] = torch.tensor(float("nan")).view(torch.int32)
    bad[2, 1] = torch.tensor(-1e30).view(torch.int32)
    gt2, n = arena.crops(desc, deg=bad, ksize=K)
    assert torch.equal(gt2, gt) and bool(torch.isnan(n[1]).all()) and bool(torch.isnan(n[2]).all())
    assert bool(torch.isfinite(n[[0] + list(range(3, B))]).all())


def test_descriptor_out_of_range_yields_nan_for_that_sample_only():
    S, scale, K = 24, 4, 21
    _, arena, batch, desc = _arena(S, scale)
    deg = _mixed_rows(len(batch), K).cuda()
    gt0, lr0 = arena.crops(desc, deg=deg, ksize=K)
    bad = desc.clone()
    bad[1] = torch.tensor([99, 0, 0, 0])
    bad[4] = torch.tensor([0, 30, 0, 0])
    bad[5] = torch.tensor([0, 0, 0, 8])
    gt, lr = arena.crops(bad, deg=deg, ksize=K)
    for i in range(len(batch)):
        if i in (1, 4, 5):
            assert bool(torch.isnan(gt[i]).all()) and bool(torch.isnan(lr[i]).all())
        else:
            assert torch.equal(gt[i], gt0[i]) and torch.equal(lr[i], lr0[i])


def test_captured_launch_replays_the_eager_bits():
    S, scale, K = 24, 4, 21
    _, arena, batch, desc = _arena(S, scale)
    deg = _mixed_rows(len(batch), K).cuda()
    gt0, lr0 = arena.crops(desc, deg=deg, ksize=K)
    gt, lr = torch.zeros_like(gt0), torch.zeros_like(lr0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, one kernel node
        arena.crops(desc, gt, lr, deg=deg, ksize=K)
    for _ in range(2):
        gt.zero_(), lr.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gt, gt0) and torch.equal(lr, lr0)
    deg.copy_(_mixed_rows(len(batch), K, noise=False).cuda())       # the graph reads deg when it runs
    graph.replay()
    assert torch.equal(lr, arena.crops(desc, deg=deg, ksize=K)[1])


def test_loader_with_a_degradation():
    """Two epochs over the small arena: gt is the loader's without the option, lr follows the restatement under the quantised rule,
    the epochs differ and an epoch repeats."""
    from srganst.device_data import Degradation, DeviceCropLoader
    S, scale, B = 24, 4, 2
    _, arena, _, _ = _arena(S, scale)
    dg = Degradation(ksize=21, blur_prob=0.8, noise_prob=0.8)
    order = list(range(len(arena)))[::-1]               # the sampler: a fixed order of the tiles
    with_deg = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=dg)
    without = DeviceCropLoader(arena, B, order, True, True, seed=2)
    assert len(with_deg) == len(without) == len(arena) // B >= 3
    seen = []
    for epoch in range(2):
        rows = with_deg.deg_draws(epoch)
        n = 0
        for (gt1, lr1), (gt0, lr0) in zip(with_deg, without):
            assert torch.equal(gt1, gt0) and tuple(lr1.shape) == tuple(lr0.shape)
            deg = rows[order[n * B:(n + 1) * B]]
            ref = refs.degrade_reference(gt1.cpu().numpy(), deg, scale, 21, quantise=False)
            refs.check_quantised(lr1.cpu().numpy(), ref, deg, f"loader epoch {epoch} batch {n}")
            seen.append(lr1.clone())
            n += 1
        assert n == len(with_deg)
    half = len(seen) // 2
    assert any(not torch.equal(a, b) for a, b in zip(seen[:half], seen[half:]))
    with_deg.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(seen[:half], with_deg))


def test_warmup_trains_on_degraded_batches(tmp_path, monkeypatch, capsys):
    import warnings
    from srganst.config import Config
    from srganst.loss import BackProjectionLoss, MSELoss
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    _, arena, _, _ = _arena(24, 4)
    cfg = Config()
    cfg.EXP.NAME, cfg.EXP.N_EPOCHS, cfg.EXP.SAVE_STATE = "degraded", 1, False
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    cfg.DATA.BATCH_SIZE, cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 2, 24, 8
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.LOG_TRAIN_PERIOD = 1
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = cfg.DATA.DEGRADE = True
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss(), "BP": BackProjectionLoss(4)}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0, "BP": 0.1}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        warmup(cfg, train_dataset=arena, test_dataset=_Pairs(), max_steps_per_epoch=2)
    assert any("BackProjectionLoss(target='gt')" in str(w.message) for w in caught)
    out = capsys.readouterr().out
    assert out.count("DATA.DEGRADE: lr = quantise") == 1 and "Degradation(blur_sigma=(0.2, 4.0)" in out
    losses = [float(v) for m in re.findall(r"\[G losses: \{([^}]*)\}", out) for v in re.findall(r": ([-+0-9.einfa]+)", m)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), out
    assert os.path.exists("results/degraded/g_last.pth")


class _TwoPairs(torch.utils.data.Dataset):
    """Two (hr, lr) pairs on the 1/255 grid, HR 128 x 112 and 104 x 120: LR sides beyond a 24-px generator tile."""

    def __init__(self):
        from srganst.bicubic import Bicubic
        g = torch.Generator().manual_seed(21)
        self.items = []
        for h, w in ((128, 112), (104, 120)):
            hr = torch.randint(0, 256, (1, 3, h, w), generator=g).float() / 255
            self.items.append((hr[0], Bicubic("cpu")(hr, scale=0.25)[0]))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_validation_on_degraded_inputs(tmp_path, capsys):
    from torch.utils.data import DataLoader
    from srganst.config import Config
    from srganst.device_data import Degradation, DeviceTestSet, degrade
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    cfg.EXP.NAME = "val"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    ds = _TwoPairs()
    params = (0.6, 3.5, 30.0, 10.0)
    want = [degrade(hr[None].cuda(), Degradation.fixed(*params, key=i).draw(1).cuda(), 4, 21) for i, (hr, _) in enumerate(ds)]
    fed = []
    hook = G.register_forward_pre_hook(lambda mod, args: fed.append(args[0].clone()))
    metrics_file = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, "val", "_metrics.txt")
    results = {}
    for on_device in (False, True):
        loader = DeviceTestSet.from_dataset(ds, "cuda") if on_device else DataLoader(ds, batch_size=1, shuffle=False)
        for tile in (0, 24):
            capsys.readouterr()
            fed.clear()
            plain = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile)
            line_plain, file_plain = capsys.readouterr().out, open(metrics_file).read()
            assert "degrade" not in line_plain and "degrade" not in file_plain and line_plain.startswith("[Test] | PSNR: ")
            if not tile:
                assert all(torch.equal(a, lr[None].cuda()) for a, (_, lr) in zip(fed, ds))
            fed.clear()
            got = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade=params)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = degrade(GT): sigma 0.6 / 3.5, theta 30 deg, noise 10 | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:                                # (tiled: the generator sees windows of the same input)
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want))
            cfg.DATA.VALIDATE_DEGRADE = params
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == got
            cfg.DATA.VALIDATE_DEGRADE = None
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == plain
            assert got != plain and all(math.isfinite(v) for v in got)
            results[on_device, tile] = (plain, got)
    hook.remove()
    for tile in (0, 24):                                 # the host and the device metric paths agree
        for a, b in zip(results[False, tile], results[True, tile]):
            assert all(abs(u - v) <= 1e-6 * abs(u) for u, v in zip(a, b))
    for on_device in (False, True):                     # the tiled forward is the whole-image forward
        for a, b in zip(results[on_device, 0], results[on_device, 24]):
            assert all(abs(u - v) <= 1e-3 * abs(u) for u, v in zip(a, b))
