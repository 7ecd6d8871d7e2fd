"""GPU: the structure-tensor maps (csrc/st_maps.hip through srganst/st.py, both radius builds) held to the fp64 oracle, and the
validation drivers' ST column.

fp64-truth rule (conftest): per output plane set  rel_err(hip, o64) <= max(1e-3, 3 rel_err(o32, o64)),
                            per-image distances   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
where o32 / l32 come from the fp32 oracle (oracle.st.st_intermediates, the reference's arithmetic: tests/test_st_maps.py holds it to
the reference's own maps) and o64 / l64 from the same oracle in fp64.  The features' references are (t, c2, s2) of the oracle's S by
the formula of st.py, in the oracle's dtype.  Every case proves from the fp64 oracle that it is not vacuous.  Single passes, nothing
captured.  Run with -s for the measured errors."""
import math
import os

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset

import st_checks
from st_checks import ALL, BUILDS
from st_checks import check_distance as _check_distance
from st_checks import features as _features
from st_checks import images as _images
from st_checks import maps_hip as _hip
from st_checks import maps_oracle as _oracle

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32, 32),      # exactly one tile
          (2, 33, 31),      # partial tiles on both axes, W not a multiple of 4
          (2, 70, 45),      # 3 x 2 tiles, ragged
          (3, 8, 8),        # smaller than the 10 / 14 px halo
          (2, 5, 3)]


# ------------------------------------------------------------------------------------------------ 1. maps against fp64
@pytest.mark.parametrize("k", range(len(SHAPES)))
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("radii", list(BUILDS))
def test_maps_vs_fp64(radii, norm, k):
    """normalize=False on [0, 1] images is degenerate (every eigenvalue of adj(S1) S2 is below 1): those inputs are on the 0..255
    scale."""
    sigma, rho = BUILDS[radii]
    B, H, W = SHAPES[k]
    x, gt = _images(300 + 10 * k + radii[0] + norm, B, H, W, scale=1.0 if norm else 255.0)
    st_checks.check_maps_vs_fp64(f"1 radii={radii} normalize={norm} {B}x{H}x{W}", x, gt, sigma, rho, norm, min_trace=5e-4)


# ------------------------------------------------------------------------------------------------ 2. 1 x 1 image
@pytest.mark.parametrize("radii", list(BUILDS))
def test_one_pixel_image(radii):
    """The centre derivative tap is 0: S is exactly 0, the features are 0 / 1e-12 = 0 and only the eps paths of the chain run,
    d = sqrt(1e-12).  The oracle gives the same on the CPU."""
    sigma, rho = BUILDS[radii]
    x, gt = torch.full((2, 3, 1, 1), 0.7), torch.full((2, 3, 1, 1), 0.2)
    o32 = _oracle(x, gt, sigma, rho, True, torch.float32)
    assert float(o32["Sx"].abs().max()) == 0 and float((o32["d"] - 1e-6).abs().max()) < 1e-12
    got = _hip(x, gt, sigma, rho)
    for key in ("Sx", "Sgt", "Fx", "Fgt"):
        assert float(got[key].abs().max()) == 0, (key, got[key])
    assert float((got["d"].double() - 1e-6).abs().max()) < 1e-12, got["d"]
    assert float((got["distance"] - 1e-6).abs().max()) < 1e-12 and tuple(got["tile_sums"].shape) == (2, 1)


# ------------------------------------------------------------------------------------------------ 3. per-image distance
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("radii", list(BUILDS))
def test_per_image_distance(radii, norm):
    from srganst import st
    from srganst.loss import StructureTensorLoss
    sigma, rho = BUILDS[radii]
    x, gt = _images(40 + radii[0] + norm, 3, 70, 45, scale=1.0 if norm else 255.0)
    x[1] = x[1] * 0.5                                   # make the images differ in more than their noise
    o32, o64 = _oracle(x, gt, sigma, rho, norm, torch.float32), _oracle(x, gt, sigma, rho, norm, torch.float64)
    assert float((o64["L"][:, 1] > 1).double().mean()) >= 0.1
    xd, gd = x.cuda(), gt.cuda()
    a = st.st_distance(xd, gd, sigma, rho, norm)
    b = st.st_distance(xd, gd, sigma, rho, norm)
    loss = StructureTensorLoss(sigma, rho, norm)(xd, gd)
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and a.is_cuda and tuple(a.shape) == (3,)
    assert torch.equal(a, b), "st_distance differs between two calls"
    a = a.cpu()
    assert len(set(a.tolist())) == 3
    name = f"3 radii={radii} normalize={norm}"
    _check_distance(name, a, o32["distance"].double(), o64["distance"])
    l32, l64 = o32["distance"].double().mean().item(), o64["distance"].mean().item()
    e, bound = abs(a.mean().item() - loss.item()), max(1e-3 * abs(l64), 3 * abs(l32 - l64))
    print(f"[{name}] batch mean {a.mean().item():.6e} vs StructureTensorLoss {loss.item():.6e}: {e:.3e} <= {bound:.3e}")
    assert e <= bound, (a.mean().item(), loss.item(), e, bound)


# ------------------------------------------------------------------------------------------------ 4. known answers
@pytest.mark.parametrize("radii", list(BUILDS))
def test_axis_convention_known_answers(radii):
    """The reference's "x" is the HEIGHT axis (utils.py:219): stripes that vary along W only have all their energy in Jyy
    (c2 = -1), along H only in Jxx (c2 = +1); sin(0.5 (col + row)) gives s2 = +1, sin(0.5 (col - row)) gives s2 = -1.  Means over the
    interior rows and columns 12..27 (away from the zero padding), within 1e-3."""
    from srganst import st
    sigma, rho = BUILDS[radii]
    r = torch.arange(40.0)[:, None].expand(40, 40)
    c = torch.arange(40.0)[None, :].expand(40, 40)
    imgs = torch.stack([torch.sin(0.5 * c), torch.sin(0.5 * r), torch.sin(0.5 * (c + r)), torch.sin(0.5 * (c - r))])
    imgs = (0.5 + 0.5 * imgs)[:, None].expand(4, 3, 40, 40).contiguous()
    expected = [(-1.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]
    o64 = _features(_oracle(imgs, imgs, sigma, rho, True, torch.float64)["Sx"])
    t, c2, s2 = st.st_features(imgs.cuda(), sigma, rho)
    S = st.structure_tensor(imgs.cuda(), sigma, rho).cpu()
    coh, ori = st.coherence(c2, s2).cpu(), st.orientation(c2, s2).cpu()
    c2, s2 = c2.cpu(), s2.cpu()
    inner = (slice(None), slice(12, 28), slice(12, 28))
    for i, (ec, es) in enumerate(expected):
        mc, ms = c2[inner][i].mean().item(), s2[inner][i].mean().item()
        print(f"[4 radii={radii}] image {i}: mean c2 {mc:+.5f} (expected {ec:+.0f})  mean s2 {ms:+.5f} (expected {es:+.0f})")
        assert abs(o64[:, 1][inner][i].mean().item() - ec) <= 1e-3 and abs(o64[:, 2][inner][i].mean().item() - es) <= 1e-3
        assert abs(mc - ec) <= 1e-3 and abs(ms - es) <= 1e-3, (i, mc, ms)
        assert abs(coh[inner][i].mean().item() - 1.0) <= 1e-3                  # one orientation only
    # plane 0 (Jxx) carries the row-to-row image, plane 1 (Jyy) the column-to-column one
    assert float(S[1, 0][12:28, 12:28].min()) > 1e3 * float(S[1, 1][12:28, 12:28].max())
    assert float(S[0, 1][12:28, 12:28].min()) > 1e3 * float(S[0, 0][12:28, 12:28].max())
    assert abs(ori[inner][1].mean().item()) <= 1e-3 and abs(ori[inner][2].mean().item() - math.pi / 4) <= 1e-3
    assert abs(ori[inner][3].mean().item() + math.pi / 4) <= 1e-3 and abs(abs(ori[inner][0]).mean().item() - math.pi / 2) <= 1e-3


# ------------------------------------------------------------------------------------------------ 5. optional outputs
@pytest.mark.parametrize("radii", list(BUILDS))
def test_optional_outputs_are_the_same_bits(radii):
    sigma, rho = BUILDS[radii]
    st_checks.check_optional_outputs_are_the_same_bits(*_images(51 + radii[0], 2, 33, 31), sigma, rho)



def test_python_surface_on_the_device():
    from srganst import st
    from srganst._abi import HipPathError
    x, gt = (t.cuda() for t in _images(7, 2, 33, 31))
    for sr_, gt_ in ((x.double(), gt.double()), (x.half(), gt), (x[0], gt[0]), (x[:, :2], gt[:, :2]), (x, gt[:, :, :30]), (x, gt.cpu())):
        with pytest.raises(HipPathError):
            st.st_distance_map(sr_, gt_)
    with pytest.raises(HipPathError, match="need gt"):
        st.st_maps(x, None, want=("Sx", "d"))
    with pytest.raises(HipPathError, match=r"radii \(4,40\)"):
        st.structure_tensor(x, sigma=1.0, rho=10.0)
    full = st.st_maps(x, gt, want=ALL)
    tracked = st.st_maps(x.clone().requires_grad_(True) * 1.0, gt, want=("d", "Sx"))     # analysis op: detached, no graph
    assert not tracked["d"].requires_grad and torch.equal(tracked["d"], full["d"]) and torch.equal(tracked["Sx"], full["Sx"])
    nc = st.st_distance_map(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), gt)       # not contiguous: made so
    assert torch.equal(nc, full["d"])
    assert torch.equal(st.st_distance_map(x, gt), full["d"]) and torch.equal(st.st_distance(x, gt), full["distance"])
    assert torch.equal(st.structure_tensor(gt), full["Sgt"])
    t, c2, s2 = st.st_features(x)
    assert torch.equal(torch.stack((t, c2, s2), dim=1), full["Fx"])


# ------------------------------------------------------------------------------------------------ 6. batch independence
@pytest.mark.parametrize("radii", list(BUILDS))
def test_batch_independence(radii):
    sigma, rho = BUILDS[radii]
    x, gt = _images(61 + radii[0], 3, 33, 31)
    x[1] = x[1] * 0.5
    batch = _hip(x, gt, sigma, rho)
    single = _hip(x[1:2].contiguous(), gt[1:2].contiguous(), sigma, rho)
    for key in ALL:
        assert torch.equal(batch[key][1], single[key][0]), f"{key} of image 1 differs between the batch and the single-image call"
    assert not torch.equal(batch["d"][0], batch["d"][1])


# ------------------------------------------------------------------------------------------------ 7. non-finite input
@pytest.mark.parametrize("radii", list(BUILDS))
def test_nan_pixel_poisons_its_neighbourhood_only(radii):
    """One NaN in sr of image 0: every S(sr) and d within Chebyshev distance R2 is NaN (the NaN-keeping clamps do not mask it);
    nothing beyond R1 + R2 (the kernel's receptive field) is touched, nor is S(gt), nor image 1."""
    sigma, rho = BUILDS[radii]
    R1, R2 = radii
    x, gt = _images(71 + radii[0], 2, 40, 40)
    y0, x0 = 17, 23
    xb = x.clone()
    xb[0, 1, y0, x0] = float("nan")
    clean, bad = _hip(x, gt, sigma, rho), _hip(xb, gt, sigma, rho)
    yy, xx = torch.meshgrid(torch.arange(40), torch.arange(40), indexing="ij")
    cheb = torch.maximum((yy - y0).abs(), (xx - x0).abs())
    near, far = cheb <= R2, cheb > R1 + R2
    assert bool(near.any()) and bool(far.any())
    assert bool(torch.isnan(bad["d"][0][near]).all()) and bool(torch.isnan(bad["Sx"][0][:, near]).all())
    assert bool(torch.isnan(bad["Fx"][0][:, near]).all())
    for key in ("d", "Sx", "Fx"):
        affected = ~torch.isfinite(bad[key][0])
        affected = affected if affected.dim() == 2 else affected.any(dim=0)
        assert not bool(affected[far].any()), f"{key}: non-finite beyond R1 + R2"
        a, b = bad[key][0][..., far], clean[key][0][..., far]
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{key}: pixels beyond R1 + R2 differ from the clean run"
    assert torch.equal(bad["Sgt"], clean["Sgt"]) and torch.equal(bad["Fgt"], clean["Fgt"])
    for key in ALL:
        assert torch.equal(bad[key][1], clean[key][1]), f"{key}: image 1 differs from the clean run"
    assert math.isnan(bad["distance"][0].item()) and math.isfinite(bad["distance"][1].item())


# ------------------------------------------------------------------------------------------------ 8. validation
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


@pytest.mark.parametrize("on_device", [False, True])
def test_validation_reports_the_st_distance(tmp_path, capsys, on_device):
    from srganst import st
    from srganst.bicubic import Bicubic
    from srganst.config import Config
    from srganst.validate import _validate, image_metrics
    cfg = Config()
    cfg.EXP.NAME = "bicubic"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    G = Bicubic(device=cfg.DEVICE).to(cfg.DEVICE)
    ds = _Pairs()
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    metrics_file = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, "bicubic", "_metrics.txt")

    # what the pass must report, from the same outputs
    psnrs, ssims, dists = [], [], []
    with torch.no_grad():
        for hr, lr in ds:
            hr, out = hr[None].cuda(), G(lr[None].cuda())
            p, s = image_metrics(out, hr)
            psnrs.append(p)
            ssims.append(s)
            dists.append(st.st_distance(out, hr).item())
    assert all(math.isfinite(v) and v > 1e-3 for v in dists) and len(set(dists)) == 3, dists

    capsys.readouterr()
    plain = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, with_st=False)
    line_plain = capsys.readouterr().out
    file_plain = open(metrics_file).read()
    default = _validate(G, loader, cfg, on_device=on_device)                    # with_st=None: the config key, off by default
    capsys.readouterr()
    with_st = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, with_st=True)
    line_st = capsys.readouterr().out
    file_st = open(metrics_file).read()
    cfg.DATA.VALIDATE_ST = True
    by_config = _validate(G, loader, cfg, on_device=on_device)
    capsys.readouterr()

    assert len(plain) == 2 and default == plain and len(with_st) == 3 and by_config == with_st
    assert with_st[:2] == plain                                                 # exactly: the option touches neither metric
    assert abs(plain[0] - sum(psnrs) / 3) <= 1e-6 and abs(plain[1] - sum(ssims) / 3) <= 1e-6
    assert with_st[2] == sum(dists) / len(dists), (with_st[2], dists)

    # with_st off: the parent's format, byte for byte
    summary = (f"[Test] | PSNR: {plain[0]:.2f} ± {_ci(psnrs):.2f} | SSIM: {plain[1]:.4f} ± {_ci(ssims):.4f} | \n")
    rows = "".join(f"{i}.png | PSNR: {p:.2f} | SSIM: {s:.4f}\n" for i, (p, s) in enumerate(zip(psnrs, ssims)))
    assert line_plain == summary + "\n"
    assert file_plain == rows + "\n" + summary + "\n"
    # with_st on: the ST column and the ST summary
    summary_st = summary[:-1] + f"ST: {with_st[2]:.4f} ± {_ci(dists):.4f} | \n"
    rows_st = "".join(f"{i}.png | PSNR: {p:.2f} | SSIM: {s:.4f} | ST: {d:.4f}\n" for i, (p, s, d) in enumerate(zip(psnrs, ssims, dists)))
    assert line_st == summary_st + "\n"
    assert file_st == rows_st + "\n" + summary_st + "\n"
    per_image = [line for line in file_st.splitlines() if ".png | PSNR:" in line]
    assert len(per_image) == 3 and all(line.count(" | ST: ") == 1 for line in per_image)      # one ST column per image ...
    assert file_st.count(" | ST: ") == 4 and line_st.count("| ST: ") == 1                     # ... and one in the summary line
    assert "ST" not in file_plain and "ST" not in line_plain
