"""CPU: the host logic of tiled whole-image inference (srganst/upscale.py) - the tile plan's properties, the receptive radius, the
inverse dihedral elements, exactness of the tiling rule on the fp64 oracle, and the index arithmetic of the uint8 gather kernel
(csrc/tiles.hip) restated in numpy."""
import itertools
import math

import numpy as np
import pytest
import torch

import upscale_refs as ur
from srganst.device_data import dihedral
from srganst.upscale import TilePlan, inverse_dihedral, receptive_radius, tiled_reference

GRID = [(H, W, tile, halo)
        for (H, W), tile, halo in itertools.product([(5, 7), (40, 40), (41, 40), (45, 70), (37, 53), (97, 101), (64, 130)],
                                                    [8, 40, 41, 64], [0, 1, 3, 10])
        if tile > 2 * halo]


@pytest.mark.parametrize("H,W,tile,halo", GRID)
def test_plan_properties(H, W, tile, halo):
    plan = TilePlan(H, W, tile, halo)
    rows = plan.rows
    assert rows.dtype == np.int32 and rows.shape == (len(plan), 6)
    assert (plan.th, plan.tw) == (min(tile, H), min(tile, W))             # one window shape per image
    count = lambda L, t: 1 if t == L else math.ceil((L - t) / (t - 2 * halo)) + 1
    assert (plan.ny, plan.nx) == (count(H, plan.th), count(W, plan.tw)) and len(plan) == plan.ny * plan.nx
    owner = np.zeros((H, W), np.int32)
    for y0, x0, oy0, oy1, ox0, ox1 in rows.tolist():
        assert 0 <= y0 and y0 + plan.th <= H and 0 <= x0 and x0 + plan.tw <= W            # every window inside the image
        assert y0 <= oy0 < oy1 <= y0 + plan.th and x0 <= ox0 < ox1 <= x0 + plan.tw        # owned inside its window, not empty
        owner[oy0:oy1, ox0:ox1] += 1
        # at least `halo` from each window edge that is not an image edge
        assert y0 == 0 and oy0 == 0 or oy0 - y0 >= halo
        assert y0 + plan.th == H and oy1 == H or y0 + plan.th - oy1 >= halo
        assert x0 == 0 and ox0 == 0 or ox0 - x0 >= halo
        assert x0 + plan.tw == W and ox1 == W or x0 + plan.tw - ox1 >= halo
    assert (owner == 1).all()                                             # the owned rectangles partition the image
    # row-major product of the two axes
    assert rows[:, 0].tolist() == sorted(rows[:, 0].tolist()) and len(set(rows[:plan.nx, 0].tolist())) == 1


def test_plan_axis_cases_and_refusal():
    assert TilePlan(30, 33, 40, 10).rows.tolist() == [[0, 0, 0, 30, 0, 33]]              # L < tile: one window owns all
    assert TilePlan(40, 40, 40, 10).rows.tolist() == [[0, 0, 0, 40, 0, 40]]              # L == tile
    p = TilePlan(41, 40, 40, 10)                                                          # L == tile + 1: two windows, one px apart
    assert p.rows.tolist() == [[0, 0, 0, 30, 0, 40], [1, 0, 30, 41, 0, 40]]
    p = TilePlan(45, 70, 40, 10)
    assert len(p) == 6 and sorted(set(p.rows[:, 1].tolist())) == [0, 20, 30]
    for tile, halo in ((20, 10), (19, 10), (1, 1)):
        with pytest.raises(ValueError, match=rf"{tile}.*{halo}"):
            TilePlan(45, 70, tile, halo)
    TilePlan(15, 15, 20, 10)                                                              # one window: the halo does not matter


def test_receptive_radius_table():
    assert [receptive_radius(*a) for a in ((16, 4), (1, 4), (2, 4), (1, 2), (16, 8))] == [40, 10, 12, 10, 40]
    with pytest.raises(ValueError):
        receptive_radius(1, 3)


def test_inverse_dihedral_on_a_rectangle():
    x = torch.arange(3 * 5 * 7).reshape(3, 5, 7)
    assert sorted(inverse_dihedral(t) for t in range(8)) == list(range(8))
    for t in range(8):
        y = dihedral(x, t)
        assert tuple(y.shape) == ((3, 7, 5) if t & 4 else (3, 5, 7))
        assert torch.equal(dihedral(y, inverse_dihedral(t)), x), t


# ---- exactness on the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rcb,upscale", [(1, 4), (2, 4), (1, 2)])
def test_tiling_rule_is_exact_on_the_fp64_oracle(n_rcb, upscale):
    fwd = ur.oracle_forward(n_rcb, upscale)
    x = ur.lr_image(45, 70)
    R = receptive_radius(n_rcb, upscale)
    with torch.no_grad():
        whole = fwd(x)
        assert ur.clamped_share(whole) < 0.01                  # the clamp would hide differences
        diff = {h: float((tiled_reference(fwd, x, TilePlan(45, 70, 40, h), upscale) - whole).abs().max()) for h in (R, R - 1, 0)}
    print(f"n_rcb {n_rcb} x{upscale}: R = {R}, max |tiled - whole| = {diff}, clamped {ur.clamped_share(whole):.4f}")
    assert diff[R] <= 1e-12
    assert diff[R - 1] > 1e-6
    assert diff[0] > 1e-2


def test_tiled_reference_ensemble_is_the_mean_over_the_eight_elements():
    fwd = ur.oracle_forward(1, 2)
    x = ur.lr_image(23, 31, seed=5)
    plan = TilePlan(23, 31, 22, 10)
    with torch.no_grad():
        got = tiled_reference(fwd, x, plan, 2, ensemble=8)
        want = sum(dihedral(fwd(dihedral(x, t).contiguous()), inverse_dihedral(t)) for t in range(8)) / 8
    assert float((got - want).abs().max()) <= 1e-12           # exact halo: tiling and the transforms commute


# ---- the uint8 gather's index arithmetic (csrc/tiles.hip: tile_gather_kernel<true> / dihedral_copy<true>) -----------------
TILE_TX, TILE_TY, TILE_TY_TR, TILE_LDS = 64, 16, 32, 3 * 64 * 33


def load_dword_unaligned(buf, a, nvalid, image_bytes):
    """pixel_io.h: bytes a .. a+3 from the one or two ALIGNED dwords that hold the first nvalid of them."""
    assert 1 <= nvalid <= 4 and 0 <= a and a + nvalid <= image_bytes         # the valid bytes are bytes of the image
    sh = a & 3
    p = a - sh
    assert p + 4 <= len(buf)                                                 # aligned load inside the padded buffer
    lo = int.from_bytes(buf[p:p + 4].tobytes(), "little")
    if sh + nvalid <= 4:
        return (lo >> (8 * sh)) & 0xFFFFFFFF
    assert p + 8 <= len(buf)
    hi = int.from_bytes(buf[p + 4:p + 8].tobytes(), "little")
    return (((hi << 32) | lo) >> (8 * sh)) & 0xFFFFFFFF


def gather_u8_restated(buf, H, W, y0w, x0w, th, tw, t):
    """One tile of sst_tile_gather from a uint8 source, workgroup by workgroup: -> uint8 [3, Ho, Wo] (the bytes the LUT is read at)."""
    tr, vf, hf = bool(t & 4), bool(t & 2), bool(t & 1)
    Ho, Wo = (tw, th) if tr else (th, tw)
    TY = TILE_TY_TR if tr else TILE_TY
    out = np.full((3, Ho, Wo), -1, np.int64)
    for y0 in range(0, Ho, TY):
        for x0 in range(0, Wo, TILE_TX):
            y1, x1 = min(y0 + TY, Ho), min(x0 + TILE_TX, Wo)
            rows, cols = y1 - y0, x1 - x0
            lo, xlo = (Ho - y1 if vf else y0), (Wo - x1 if hf else x0)
            nrow, seg = (cols, rows) if tr else (rows, cols)
            sy0, sx0 = y0w + (xlo if tr else lo), x0w + (lo if tr else xlo)
            segb = 3 * seg
            ndw = (segb + 3) >> 2
            P = ndw | 1
            assert nrow * P <= TILE_LDS
            lds = np.zeros(nrow * P * 4, np.uint8)
            base, rowb = (sy0 * W + sx0) * 3, 3 * W
            for row in range(nrow):
                for k in range(ndw):
                    v = load_dword_unaligned(buf, base + row * rowb + 4 * k, min(4, segb - 4 * k), H * W * 3)
                    lds[(row * P + k) * 4:(row * P + k) * 4 + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)
            for c in range(3):
                for r in range(rows):
                    for x in range(cols):
                        line = ((Ho - 1 - (y0 + r)) if vf else y0 + r) - lo
                        xm = ((Wo - 1 - (x0 + x)) if hf else x0 + x) - xlo
                        row, k = (xm, line) if tr else (line, xm)
                        out[c, y0 + r, x0 + x] = lds[row * P * 4 + k * 3 + c]
    assert (out >= 0).all()
    return out.astype(np.uint8)


@pytest.mark.parametrize("H,W,th,tw,windows", [
    (37, 53, 16, 24, [(0, 0), (5, 7), (21, 29), (3, 29), (21, 1)]),        # odd x0; windows that end at the last row and column
    (41, 150, 40, 131, [(1, 19), (0, 0)]),                                   # several workgroups per tile on both axes
])
def test_uint8_gather_index_arithmetic(H, W, th, tw, windows):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    n = H * W * 3
    buf = np.full((n + 15) & ~15, 255, np.uint8)                              # the padding is never part of a result
    buf[:n] = img.reshape(-1)
    x = torch.from_numpy(img).permute(2, 0, 1)
    for t in range(8):
        for y0, x0 in windows:
            want = dihedral(x[:, y0:y0 + th, x0:x0 + tw], t)                  # tiled_reference's window, transformed
            got = gather_u8_restated(buf, H, W, y0, x0, th, tw, t)
            assert np.array_equal(got, want.numpy()), (t, y0, x0)
