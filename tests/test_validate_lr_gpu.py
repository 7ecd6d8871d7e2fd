"""GPU: validation with the LR-consistency column (validate --lr-consistency, DATA.VALIDATE_LR): a three-image synthetic test set
with Bicubic as "generator" and with a two-block Generator.  The column is metrics.lr_consistency of each output against the
loader's own LR image, as an LR-PSNR; the host and the device metric paths agree; the return tuple follows the two flags; with the
option off the pass writes what it wrote before the option existed."""
import math
import os

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset

pytestmark = pytest.mark.gpu


class _Pairs(Dataset):
    """Three (hr, lr) pairs on the 1/255 grid, HR 96 x 80 and 64 x 72."""

    def __init__(self):
        from srganst.bicubic import Bicubic
        g = torch.Generator().manual_seed(9)
        self.items = []
        for h, w in ((96, 80), (64, 72), (96, 80)):
            base = torch.rand(1, 3, h // 8, w // 8, generator=g)
            hr = torch.round(F.interpolate(base, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1) * 255) / 255
            self.items.append((hr[0], Bicubic("cpu")(hr, scale=0.25)[0]))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _ci(data):
    from srganst.validate import confidence_interval
    return confidence_interval(data)


def _generator(kind, cfg):
    if kind == "bicubic":
        from srganst.bicubic import Bicubic
        return Bicubic(device=cfg.DEVICE).to(cfg.DEVICE)
    from srganst.model import Generator
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 2
    torch.manual_seed(3)
    return Generator(cfg).to(cfg.DEVICE).eval()


@pytest.mark.parametrize("kind", ["bicubic", "generator"])
def test_validation_reports_the_lr_psnr(tmp_path, capsys, kind):
    from srganst import st
    from srganst.config import Config
    from srganst.metrics import lr_consistency, lr_psnr_from_mse
    from srganst.validate import _validate, image_metrics
    cfg = Config()
    assert cfg.DATA.VALIDATE_LR is False
    cfg.EXP.NAME = kind
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    G = _generator(kind, cfg)
    ds = _Pairs()
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    metrics_file = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, kind, "_metrics.txt")

    # what the pass must report, from the same outputs: lr_consistency called by hand
    psnrs, ssims, dists, lrs = [], [], [], []
    with torch.no_grad():
        for hr, lr in ds:
            hr, lr = hr[None].cuda(), lr[None].cuda()
            out = G(lr)
            p, s = image_metrics(out, hr)
            psnrs.append(p)
            ssims.append(s)
            dists.append(st.st_distance(out, hr).item())
            lrs.append(lr_psnr_from_mse(lr_consistency(out, lr, 4).item()))
    assert all(math.isfinite(v) for v in lrs) and len(set(lrs)) == 3, lrs
    print(f"[validate {kind}] LR-PSNR per image {lrs}")

    runs = {}
    for on_device in (False, True):
        capsys.readouterr()
        plain = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, with_st=False, with_lr=False)
        line_plain = capsys.readouterr().out
        file_plain = open(metrics_file).read()
        default = _validate(G, loader, cfg, on_device=on_device)                # with_lr=None: the config key, off by default
        capsys.readouterr()
        with_lr = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, with_lr=True)
        line_lr = capsys.readouterr().out
        file_lr = open(metrics_file).read()
        with_st = _validate(G, loader, cfg, on_device=on_device, with_st=True)
        capsys.readouterr()
        both = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, with_st=True, with_lr=True)
        line_both = capsys.readouterr().out
        file_both = open(metrics_file).read()
        cfg.DATA.VALIDATE_LR = True
        by_config = _validate(G, loader, cfg, on_device=on_device)
        cfg.DATA.VALIDATE_LR = False
        capsys.readouterr()
        runs[on_device] = with_lr

        # the return tuple in all four flag combinations
        assert len(plain) == 2 and default == plain and len(with_lr) == 3 and len(with_st) == 3 and len(both) == 4
        assert by_config == with_lr and with_lr[:2] == plain and with_st[:2] == plain and both[:3] == with_st and both[3] == with_lr[2]
        assert with_lr[2] == sum(lrs) / 3, (with_lr[2], lrs)                    # lr_consistency called by hand, the same bits
        assert abs(with_st[2] - sum(dists) / 3) <= 1e-9 * with_st[2]

        # the option off: today's format, byte for byte, from image_metrics
        summary = (f"[Test] | PSNR: {plain[0]:.2f} ± {_ci(psnrs):.2f} | SSIM: {plain[1]:.4f} ± {_ci(ssims):.4f} | \n")
        rows = "".join(f"{i}.png | PSNR: {p:.2f} | SSIM: {s:.4f}\n" for i, (p, s) in enumerate(zip(psnrs, ssims)))
        assert line_plain == summary + "\n"
        assert file_plain == rows + "\n" + summary + "\n"
        assert "LR-PSNR" not in file_plain and "LR-PSNR" not in line_plain
        # on: the column and its summary; after ST when both are on
        summary_lr = summary[:-1] + f"LR-PSNR: {with_lr[2]:.2f} ± {_ci(lrs):.2f} | \n"
        rows_lr = "".join(f"{i}.png | PSNR: {p:.2f} | SSIM: {s:.4f} | LR-PSNR: {v:.2f}\n" for i, (p, s, v) in enumerate(zip(psnrs, ssims, lrs)))
        assert line_lr == summary_lr + "\n"
        assert file_lr == rows_lr + "\n" + summary_lr + "\n"
        assert file_lr.count(" | LR-PSNR: ") == 4 and line_lr.count("| LR-PSNR: ") == 1
        summary_both = summary[:-1] + f"ST: {both[2]:.4f} ± {_ci(dists):.4f} | LR-PSNR: {both[3]:.2f} ± {_ci(lrs):.2f} | \n"
        rows_both = "".join(f"{i}.png | PSNR: {p:.2f} | SSIM: {s:.4f} | ST: {d:.4f} | LR-PSNR: {v:.2f}\n"
                            for i, (p, s, d, v) in enumerate(zip(psnrs, ssims, dists, lrs)))
        assert line_both == summary_both + "\n"
        assert file_both == rows_both + "\n" + summary_both + "\n"

    # the host and the device metric paths agree
    assert abs(runs[True][2] - runs[False][2]) <= 1e-9 * abs(runs[False][2])
