"""GPU: tiled whole-image inference (srganst/upscale.py, csrc/tiles.hip).  The three kernels against plain-torch restatements bit
for bit, the Upscaler against the fp64 oracle with the whole-image HIP forward as the yardstick, the uint8 path, the command line
and validation with DATA.VALIDATE_TILE."""
import numpy as np
import pytest
import torch

import upscale_refs as ur

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP_AT_ONE = 2.0 ** -23
TRUTH_FACTOR = 3.0            # conftest.TRUTH_FACTOR: the project's factor on the reference arithmetic's own error


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_values(a, b):
    """Equal where neither is NaN, NaN in the same places (an addition need not keep a NaN's payload)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def padded_u8(img):
    """uint8 [H,W,3] -> the flat device buffer sst_tile_gather takes: padded to a multiple of 16 bytes (with 255s: never part of a result)."""
    flat = torch.as_tensor(np.ascontiguousarray(img)).reshape(-1)
    buf = torch.full(((flat.numel() + 15) & ~15,), 255, dtype=torch.uint8)
    buf[:flat.numel()] = flat
    return buf.to(DEV)


# ---- gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,th,tw,windows", [
    (37, 53, 16, 24, [(0, 0), (5, 7), (21, 29), (3, 29), (21, 1)]),        # odd x0; windows that end at the last row and column
    (41, 150, 40, 131, [(1, 19), (0, 0)]),                                   # several workgroups per tile on both axes
])
def test_gather_equals_the_restatement(H, W, th, tw, windows):
    from srganst.device_data import dihedral, lut
    from srganst.upscale import tile_gather
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    chw = img.permute(2, 0, 1).contiguous()
    src8, src32, table = padded_u8(img), (chw.float() / 255.0).to(DEV), lut(DEV)
    for t in range(8):
        want = torch.stack([dihedral(chw[:, y0:y0 + th, x0:x0 + tw], t).contiguous().float() / 255.0 for y0, x0 in windows])
        desc = torch.tensor([(y0, x0, t) for y0, x0 in windows], dtype=torch.int32, device=DEV)
        got8 = tile_gather(src8, H, W, desc, th, tw, t, table).cpu()
        got32 = tile_gather(src32, H, W, desc, th, tw, t).cpu()
        assert same_bits(got8, want), f"uint8 source, t={t}"
        assert same_bits(got32, want), f"fp32 source, t={t}"


def test_gather_descriptor_outside_the_image_yields_nan():
    from srganst.device_data import lut
    from srganst.upscale import tile_gather
    H, W, th, tw = 37, 53, 16, 24
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    src8, src32 = padded_u8(img), (img.permute(2, 0, 1).float() / 255.0).contiguous().to(DEV)
    bad = [(22, 0, 5), (0, 30, 5), (-1, 0, 5), (0, -1, 5), (2 ** 31 - 8, 0, 5), (0, 0, 4), (0, 0, 13)]   # the last two: another t
    desc = torch.tensor([(3, 5, 5)] + bad, dtype=torch.int32, device=DEV)
    for src, table in ((src8, lut(DEV)), (src32, None)):
        out = tile_gather(src, H, W, desc, th, tw, 5, table).cpu()
        assert not out[0].isnan().any()
        assert out[1:].isnan().all()


# ---- scatter and quantiser --------------------------------------------------------------------------------------------------
def awkward_tiles(shape, seed):
    """Values below 0, above 1, exactly (k + 0.5) / 255 and NaN among ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 2.0 - 0.5
    kind = torch.randint(0, 8, shape, generator=g)
    half = (torch.randint(0, 255, shape, generator=g).float() + 0.5) / 255.0
    v = torch.where(kind == 0, half, v)
    return torch.where(torch.rand(shape, generator=g) < 0.002, torch.full(shape, float("nan")), v)


def scatter_restated(canvas, tiles, rows, th, tw, s, t, accumulate):
    from srganst.device_data import dihedral
    from srganst.upscale import inverse_dihedral
    for b, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(rows.tolist()):
        u = dihedral(tiles[b], inverse_dihedral(t))
        assert tuple(u.shape) == (3, s * th, s * tw)
        piece = u[:, s * (oy0 - y0):s * (oy1 - y0), s * (ox0 - x0):s * (ox1 - x0)]
        dst = canvas[:, s * oy0:s * oy1, s * ox0:s * ox1]
        dst.copy_(dst + piece if accumulate else piece)
    return canvas


@pytest.mark.parametrize("H,W,tile,halo,s", [(37, 53, 24, 3, 4), (21, 53, 24, 5, 2), (9, 150, 80, 2, 4)])
def test_scatter_and_quantiser_equal_the_restatement(H, W, tile, halo, s):
    from srganst.upscale import TilePlan, canvas_to_u8, tile_scatter
    from srganst.utils import tensor2img
    plan = TilePlan(H, W, tile, halo)
    th, tw = plan.th, plan.tw
    keep = np.ones(len(plan), bool)
    keep[len(plan) // 2] = False                                              # one window's rectangle stays unowned
    rows_host = torch.from_numpy(plan.rows[keep])
    rows = rows_host.to(DEV)
    B = len(rows_host)
    SENTINEL = -7.25
    acc_ref = acc = None
    for t in range(8):
        Ho, Wo = (tw, th) if t & 4 else (th, tw)
        tiles = awkward_tiles((B, 3, s * Ho, s * Wo), seed=10 + t)
        # store mode into a sentinel-filled canvas
        ref = scatter_restated(torch.full((3, s * H, s * W), SENTINEL), tiles, rows_host, th, tw, s, t, False)
        got = tile_scatter(tiles.to(DEV), rows, H, W, th, tw, s, t, torch.full((3, s * H, s * W), SENTINEL, device=DEV)).cpu()
        assert same_bits(got, ref), f"store, t={t}"
        y0, x0, oy0, oy1, ox0, ox1 = plan.rows[len(plan) // 2].tolist()
        assert (got[:, s * oy0:s * oy1, s * ox0:s * ox1] == SENTINEL).all()      # pixels that no row owns keep the sentinel
        assert ref.isnan().any() and (ref[~ref.isnan()] < 0).any() and (ref > 1).any()
        # eight accumulations: the first pass stores, the others add
        if t == 0:
            acc_ref, acc = ref.clone(), got.clone().to(DEV)
        else:
            acc_ref = scatter_restated(acc_ref, tiles, rows_host, th, tw, s, t, True)
            tile_scatter(tiles.to(DEV), rows, H, W, th, tw, s, t, acc, accumulate=True)
        if t == 0:
            q = canvas_to_u8(got.to(DEV)).cpu()
            nan = ref.isnan().any(0)
            want = torch.from_numpy(np.ascontiguousarray(tensor2img(ref.nan_to_num(0.0))[..., ::-1]))     # BGR -> RGB
            assert q.dtype == torch.uint8 and tuple(q.shape) == (s * H, s * W, 3)
            assert torch.equal(q, want)                                        # NaN -> 0 as well: nan_to_num made them 0
            assert (q.permute(2, 0, 1)[ref.isnan()] == 0).all() and nan.any()
    assert same_values(acc.cpu(), acc_ref), "after eight accumulations"
    q8 = canvas_to_u8(acc, 0.125).cpu()
    want8 = torch.from_numpy(np.ascontiguousarray(tensor2img((acc_ref * 0.125).nan_to_num(0.0))[..., ::-1]))
    assert torch.equal(q8, want8)


def test_quantiser_on_a_canvas_whose_planes_are_not_16_byte_aligned():
    from srganst.upscale import canvas_to_u8
    from srganst.utils import tensor2img
    c = awkward_tiles((3, 5, 7), seed=3)
    c[1, 2, 3] = float("nan")
    q = canvas_to_u8(c.to(DEV)).cpu()
    want = torch.from_numpy(np.ascontiguousarray(tensor2img(c.nan_to_num(0.0))[..., ::-1]))
    assert torch.equal(q, want) and q[2, 3, 1] == 0


# ---- pipeline ---------------------------------------------------------------------------------------------------------------
def hip_generator(n_rcb, upscale):
    from srganst.config import Config
    from srganst.model import Generator
    cfg = Config()
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.DATA.UPSCALE_FACTOR = ur.CH, n_rcb, upscale
    G = Generator(cfg)
    G.load_state_dict(ur.generator_state(n_rcb, upscale))
    return G.to(DEV).eval()


_CACHE = {}


def whole_image(n_rcb, upscale, H, W):
    """(generator, x fp32 on the device, oracle fp64 whole-image result, e(whole-image HIP forward)) - computed once per case."""
    key = (n_rcb, upscale, H, W)
    if key not in _CACHE:
        G = hip_generator(n_rcb, upscale)
        x64 = ur.lr_image(H, W).float().double()                   # fp32 values: the oracle and the device see the same input
        with torch.no_grad():
            truth = ur.oracle_forward(n_rcb, upscale)(x64)
            x = x64.float().to(DEV)
            whole = G(x)
        assert ur.clamped_share(truth) < 0.01
        _CACHE[key] = (G, x, truth, whole, float((whole.cpu().double() - truth).abs().max()))
    return _CACHE[key]


@pytest.mark.parametrize("n_rcb,upscale,H,W", [(1, 4, 45, 70), (1, 2, 45, 70), (1, 4, 21, 70)])
def test_tiled_forward_is_the_whole_image_forward(n_rcb, upscale, H, W):
    from srganst.upscale import Upscaler, receptive_radius
    G, x, truth, _, e_whole = whole_image(n_rcb, upscale, H, W)
    err = lambda y: float((y.cpu().double() - truth).abs().max())
    up = Upscaler(G, tile=40, batch=4)
    assert up.halo == receptive_radius(n_rcb, upscale) == 10
    plan = up.plan(H, W)
    assert len(plan) == (6 if H == 45 else 3) and (plan.th, plan.tw) == (min(H, 40), 40)       # 45 x 70: six tiles run as 4 + 2
    sr = up(x)
    assert tuple(sr.shape) == (1, 3, upscale * H, upscale * W)
    bound = max(TRUTH_FACTOR * e_whole, ULP_AT_ONE)
    e_tiled, e_halo0 = err(sr), err(Upscaler(G, tile=40, halo=0, batch=4)(x))
    print(f"n_rcb {n_rcb} x{upscale} {H}x{W}: e(whole) {e_whole:.3e}, e(tiled) {e_tiled:.3e}, bound {bound:.3e}, e(halo 0) {e_halo0:.3e}")
    assert e_tiled <= bound
    assert e_halo0 > 100 * bound


def test_tiled_self_ensemble_against_the_reference():
    from srganst.upscale import Upscaler, tiled_reference
    G, x, _, _, e_whole = whole_image(1, 4, 21, 70)
    up = Upscaler(G, tile=40, batch=2, ensemble=8)                  # three 21 x 40 windows as 2 + 1; transposed passes run 40 x 21
    with torch.no_grad():
        truth = tiled_reference(ur.oracle_forward(1, 4), x.cpu().double(), up.plan(21, 70), 4, ensemble=8)
    sr = up(x)
    bound = max(TRUTH_FACTOR * e_whole, ULP_AT_ONE)
    e = float((sr.cpu().double() - truth).abs().max())
    print(f"ensemble 8: e {e:.3e}, bound {bound:.3e}")
    assert e <= bound


def test_image_that_fits_one_window_is_the_plain_forward():
    from srganst.upscale import Upscaler
    G, x, _, whole, _ = whole_image(1, 4, 30, 33)
    assert torch.equal(Upscaler(G, tile=40)(x), whole)


def test_upscaler_refuses_what_it_cannot_do():
    from srganst.upscale import Upscaler
    G = hip_generator(1, 4)
    with pytest.raises(ValueError, match="eval"):
        Upscaler(G.train())
    G.eval()
    with pytest.raises(ValueError, match="ensemble"):
        Upscaler(G, ensemble=4)
    with pytest.raises(ValueError, match=r"20.*10"):
        Upscaler(G, tile=20)(torch.zeros(1, 3, 45, 70, device=DEV))
    # B * (4*th) * (4*tw) * 16 / 4 < 2^29: 2^28 elements per 2048 x 2048 window, 2^30 per 4096 x 4096 window
    assert Upscaler(G, tile=2048, batch=8).batch_for(2048, 2048) == 1 and Upscaler(G, tile=64).batch_for(64, 64) == 8
    with pytest.raises(ValueError, match="smaller tile"):
        Upscaler(G, tile=4096).batch_for(4096, 4096)


# ---- uint8 ------------------------------------------------------------------------------------------------------------------
def test_uint8_path_against_the_whole_image_forward():
    from srganst.upscale import Upscaler
    from srganst.utils import tensor2img
    G = hip_generator(1, 4)
    img = torch.randint(0, 256, (45, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    x = (img.permute(2, 0, 1).float() / 255.0).unsqueeze(0).contiguous().to(DEV)
    up = Upscaler(G, tile=40, batch=4)
    with torch.no_grad():
        whole = G(x)
    d = float((up(x) - whole).abs().max())                                  # measured max |tiled - whole|
    got = up.upscale_u8(img.numpy()).cpu().numpy().astype(np.int64)
    want = tensor2img(whole)[..., ::-1].astype(np.int64)                    # BGR -> RGB
    assert got.shape == (180, 280, 3)
    assert np.abs(got - want).max() <= 1
    v = whole[0].permute(1, 2, 0).cpu().double().numpy() * 255.0
    safe = np.abs(v - np.floor(v) - 0.5) > 255.0 * d                        # farther than 255 d from a half-integer
    print(f"uint8: d = {d:.3e}, {int((got != want).sum())} of {got.size} levels differ, {int((~safe).sum())} within 255 d of a half")
    assert np.array_equal(got[safe], want[safe])


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_upscaled_images(tmp_path, capsys):
    from PIL import Image
    from srganst import upscale
    G = hip_generator(1, 4)
    torch.save(G.state_dict(), tmp_path / "g.pth")
    g = torch.Generator().manual_seed(4)
    arrays = {"a.png": torch.randint(0, 256, (30, 33, 3), dtype=torch.uint8, generator=g).numpy(),
              "b.png": torch.randint(0, 256, (45, 70, 3), dtype=torch.uint8, generator=g).numpy()}
    (tmp_path / "in").mkdir()
    for name, a in arrays.items():
        Image.fromarray(a).save(tmp_path / "in" / name)
    upscale.main(["--g-path", str(tmp_path / "g.pth"), "--in-dir", str(tmp_path / "in"), "--out-dir", str(tmp_path / "out"),
                  "--tile", "40", "--batch", "4"])
    assert "images/s" in capsys.readouterr().out
    up = upscale.Upscaler(G, tile=40, batch=4)
    for name, a in arrays.items():
        out = np.asarray(Image.open(tmp_path / "out" / name).convert("RGB"))
        assert out.shape == (4 * a.shape[0], 4 * a.shape[1], 3)
        assert np.array_equal(out, up.upscale_u8(a).cpu().numpy())


# ---- validation ---------------------------------------------------------------------------------------------------------------
def test_validate_tile_on_images_that_fit_one_window(monkeypatch):
    from torch.utils.data import DataLoader
    from srganst import upscale
    from srganst.config import Config
    from srganst.validate import _validate
    G = hip_generator(1, 4)
    g = torch.Generator().manual_seed(6)
    pairs = [(torch.rand(3, 4 * h, 4 * w, generator=g), torch.rand(3, h, w, generator=g)) for h, w in ((30, 33), (12, 40), (17, 23))]
    loader = DataLoader(pairs, batch_size=1, shuffle=False)
    cfg = Config()
    cfg.DEVICE = DEV
    assert cfg.DATA.VALIDATE_TILE == 0
    plain = _validate(G, loader, cfg)
    calls = []
    call = upscale.Upscaler.__call__
    monkeypatch.setattr(upscale.Upscaler, "__call__", lambda self, lr: (calls.append(tuple(lr.shape)), call(self, lr))[1])
    cfg.DATA.VALIDATE_TILE = 40
    tiled = _validate(G, loader, cfg)
    assert len(calls) == 3                                                   # the generator ran through the Upscaler
    assert tiled == plain
    assert _validate(G, loader, cfg, tile=0) == plain and len(calls) == 3
