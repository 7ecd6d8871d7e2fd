"""GPU: the random resize of the first degradation stage (csrc/resize.hip: sst_rescale_to; csrc/degrade.hip: sst_blur;
srganst.device_data: rescale_to, blur, degrade(resize_rows=...), Degradation(resize_prob=...), DeviceCropLoader; validate's
degrade_resize1) against the fp64 restatement of tests/resize1_refs.py and its derived bound.

Measured on one MI355X, max |kernel - restatement| before quantisation and the worst ratio to the sample's bound, per shape: DESIGN.md
section 25 has the table."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import resize1_refs as refs
from test_degrade_gpu import _TwoPairs, _arena

pytestmark = pytest.mark.gpu

SHAPES = [((8, 8), (2, 2)), ((12, 20), (3, 5)), ((36, 44), (9, 11)), ((50, 70), (12, 17)), ((14, 10), (7, 5)), ((64, 72), (8, 9)),
          ((132, 40), (33, 10)), ((96, 96), (24, 24))]
up8 = lambda n: -(-n // 8)
up4 = lambda n: -(-n // 4)


def _size(kind, H, W):
    if kind is None:
        return None
    return {"same": (H, W), "min": (up8(H), up8(W)), "max": (2 * H, 2 * W), "p15": (max(int(0.15 * H), up8(H)), max(int(0.15 * W), up8(W))),
            "frac": (max(int(0.77 * H), up8(H)), max(int(0.77 * W), up8(W))),
            "aniso": (min(2 * H, H + max(1, H // 3)), max(up8(W), W - max(1, W // 3)))}[kind]


def _rows(spec, H, W, keys=None):
    """[(size kind or None, m1, m2, noise255, shot, gray, key)] -> int32 [n, 8]."""
    from srganst.device_data import rescale_rows
    return torch.from_numpy(rescale_rows([_size(s[0], H, W) for s in spec], [(s[1], s[2]) for s in spec], [s[3] for s in spec],
                                         [s[4] for s in spec], [s[5] for s in spec],
                                         keys or [(s[6], s[6] * 7919 + 1) for s in spec]))


# the row sets of the restatement cases, B = 1 and B = 3: keep, ceil(H / 8), 2 H, int(0.15 H) raised to the limit, int(0.77 H), an
# anisotropic pair (rows up, columns down), the nine mode pairs, noise off / colour / gray / shot
ROW_SETS = [
    [("frac", "bicubic", "bilinear", 10.0, 0.01, 1, 11)],
    [("p15", "area", "bicubic", 6.0, 0.0, 0, 13)],
    [(None, "area", "area", 0.0, 0.0, 0, 1), (None, "area", "bicubic", 20.0, 0.0, 0, 2), ("same", "bicubic", "bicubic", 20.0, 0.0, 0, 2)],
    [("min", "area", "area", 0.0, 0.0, 0, 3), ("max", "bilinear", "bilinear", 5.0, 0.0, 0, 4), ("frac", "bicubic", "area", 0.0, 0.02, 1, 5)],
    [("aniso", "area", "bilinear", 8.0, 0.01, 0, 6), ("p15", "bilinear", "area", 0.0, 0.0, 0, 7), ("max", "bicubic", "area", 3.0, 0.0, 1, 8)],
    [("min", "bilinear", "bicubic", 12.0, 0.0, 0, 9), ("aniso", "bicubic", "bilinear", 0.0, 0.0, 0, 10), (None, "area", "bilinear", 0.0, 0.01, 1, 12)],
]
assert {(s[1], s[2]) for rs in ROW_SETS for s in rs if s[0]} == {(a, b) for a in refs.MODES for b in refs.MODES}


@functools.lru_cache(maxsize=None)
def _input(B, H, W):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
    return torch.rand(B, 3, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(H, W, h, w, which):
    """The unquantised fp64 restatement of one row set on the shared input: computed once, read by every test that needs it."""
    rows = _rows(ROW_SETS[which], H, W)
    ref = refs.rescale_to_reference(_input(len(rows), H, W).numpy(), rows.numpy(), (h, w), quantise=False)
    ref.setflags(write=False)
    return ref


def _run(x, rows, size, **kw):
    from srganst.device_data import rescale_to
    return rescale_to(x.cuda(), rows.cuda(), size, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid(raw):
    return torch.round(255 * raw.clamp(0, 1)) / 255


@pytest.mark.parametrize("big, small", SHAPES)
def test_kernel_against_the_restatement(big, small):
    """Per sample: the unquantised output within the derived bound of the restatement; the quantised output = round(255 clamp(v)) / 255
    taken in fp32 from the unquantised launch."""
    (H, W), (h, w) = big, small
    worst, worst_abs = 0.0, 0.0
    for which, spec in enumerate(ROW_SETS):
        rows, x = _rows(spec, H, W), _input(len(spec), H, W)
        raw = _run(x, rows, small, quantise=False).cpu()
        assert tuple(raw.shape) == (len(spec), 3, h, w)
        ref, bound = _reference(H, W, h, w, which), refs.bound(rows.numpy(), H, W, h, w)
        q = _run(x, rows, small).cpu()
        for b, s in enumerate(spec):
            err = float(np.abs(raw[b].double().numpy() - ref[b]).max())
            worst, worst_abs = max(worst, err / bound[b]), max(worst_abs, err)
            print(f"rescale_to {H}x{W} -> {h}x{w} rows {which}[{b}] {s[0]} {_size(s[0], H, W)} {s[1]}/{s[2]}: max |kernel - fp64| = "
                  f"{err:.3g}, bound {bound[b]:.3g}")
            assert err <= bound[b], (which, b, err, bound[b])
            assert torch.equal(q[b], _grid(raw[b])), (which, b)
            assert float(q[b].min()) >= 0 and float(q[b].max()) <= 1
    print(f"rescale_to {H}x{W} -> {h}x{w}: worst error {worst_abs:.3g}, worst error / bound = {worst:.3f}")


def _size24(kind, h, w):
    if kind is None:
        return None
    return {"same": (h, w), "min": (up4(h), up4(w)), "max": (2 * h, 2 * w), "frac": (max(int(0.77 * h), up4(h)), max(int(0.77 * w), up4(w))),
            "aniso": (min(2 * h, h + max(1, h // 3)), max(up4(w), w - max(1, w // 3)))}[kind]


@pytest.mark.parametrize("h, w", [(7, 9), (33, 40), (65, 31)])
def test_equal_geometry_gives_rescale_s_bits(h, w):
    """At (H, W) == (h, w) every row that sst_rescale accepts gives sst_rescale's bits: pass-through (NaNs, infinities and a NaN payload
    included), noise alone, the image's own size, the smallest and the largest size of section 24, a non-integer ratio, an
    anisotropic pair, the nine mode pairs, colour, gray and shot noise; and the rows it refuses for a reason other than its size
    limit are NaN here too."""
    from srganst.device_data import rescale, rescale_rows, rescale_to
    spec = [(None, "area", "area", 0.0, 0.0, 0), (None, "bicubic", "bilinear", 0.0, 0.0, 1), (None, "area", "area", 20.0, 0.0, 0),
            (None, "bilinear", "area", 0.0, 0.02, 1), ("same", "bicubic", "bicubic", 20.0, 0.0, 0), ("same", "area", "bilinear", 0.0, 0.0, 0),
            ("min", "area", "area", 0.0, 0.0, 0), ("max", "bilinear", "bilinear", 5.0, 0.0, 0), ("frac", "bicubic", "area", 0.0, 0.02, 1),
            ("aniso", "area", "bilinear", 8.0, 0.01, 0), ("frac", "area", "bicubic", 0.0, 0.0, 0), ("max", "bilinear", "area", 3.0, 0.0, 1),
            ("min", "bilinear", "bicubic", 12.0, 0.0, 0), ("aniso", "bicubic", "bilinear", 0.0, 0.0, 0), ("max", "bicubic", "bicubic", 0.0, 0.0, 0),
            ("min", "bicubic", "area", 4.0, 0.0, 0)]
    n = len(spec)
    rows = torch.from_numpy(rescale_rows([_size24(s[0], h, w) for s in spec], [(s[1], s[2]) for s in spec], [s[3] for s in spec],
                                         [s[4] for s in spec], [s[5] for s in spec], [(i + 1, 7919 * i + 3) for i in range(n)]))
    bad = rows[:5].clone()
    bad[0, 6], bad[1, 0], bad[2, 2], bad[3, 6], bad[4, 1] = 3, -3, int(np.float32(-1.0).view(np.int32)), 1 << 5, 0
    rows = torch.cat([rows, bad]).cuda()
    x = ((_input(n + 5, h, w) - 0.25) * 2).cuda()
    x[0, 1, 3, 5], x[0, 2, h - 1, w - 1], x[1, 0, 0, 0] = float("nan"), float("inf"), float("-inf")
    _bits(x)[0, 0, 0, 1] = 0x7FC01234
    for quantise in (True, False):
        want = rescale(x, rows, quantise=quantise)
        got = rescale_to(x, rows, (h, w), quantise=quantise)
        assert torch.equal(_bits(got), _bits(want)), quantise
        assert torch.equal(_bits(got[:2]), _bits(x[:2])) and bool(torch.isnan(got[n:]).all()) and bool(torch.isfinite(got[2:n]).all())


def test_a_constant_image_comes_back_constant():
    (H, W), (h, w) = (36, 44), (9, 11)
    x = torch.empty(3, 3, H, W)
    x[0], x[1], x[2] = 100 / 255, 1.0, 0.0
    want = x[:, :, :h, :w]
    for m1 in refs.MODES:
        for m2 in refs.MODES:
            for kind in (None, "min", "p15", "frac", "max", "aniso"):
                rows = _rows([(kind, m1, m2, 0.0, 0.0, 0, 1)] * 3, H, W)
                assert torch.equal(_run(x, rows, (h, w)).cpu(), want), (m1, m2, kind)
                raw = _run(x, rows, (h, w), quantise=False).cpu()
                assert float((raw - want).abs().max()) <= refs.bound(rows.numpy(), H, W, h, w).max()


def test_a_sample_sees_its_key_but_neither_its_position_the_batch_nor_the_tiles(monkeypatch):
    from srganst.device_data import rescale_to
    (H, W), size = (50, 70), (12, 17)
    spec = [("frac", "bicubic", "bilinear", 8.0, 0.0, 0, 1), (None, "area", "area", 0.0, 0.0, 0, 2), ("max", "area", "bicubic", 0.0, 0.02, 1, 3),
            ("min", "bilinear", "area", 12.0, 0.0, 0, 4), (None, "area", "bicubic", 9.0, 0.01, 0, 5), ("aniso", "bicubic", "area", 0.0, 0.0, 0, 6)]
    x, rows = _input(6, H, W).cuda(), _rows(spec, H, W).cuda()
    a = rescale_to(x, rows, size)
    assert torch.equal(rescale_to(x, rows, size), a)                                # same inputs, same bits
    perm = torch.tensor([3, 0, 5, 4, 1, 2], device="cuda")
    assert torch.equal(rescale_to(x[perm].contiguous(), rows[perm].contiguous(), size), a[perm])
    for b in (0, 2, 3):
        assert torch.equal(rescale_to(x[b:b + 1].contiguous(), rows[b:b + 1].contiguous(), size)[0], a[b])
    assert torch.equal(rescale_to(x[:3].contiguous(), rows[:3].contiguous(), size), a[:3])
    rekeyed = rows.clone()
    rekeyed[:, 4] += 1
    b = rescale_to(x, rekeyed, size)
    assert torch.equal(b[1], a[1]) and torch.equal(b[5], a[5]) and all(not torch.equal(b[i], a[i]) for i in (0, 2, 3, 4))
    raw = rescale_to(x, rows, size, quantise=False)
    for tile in ("8x8", "4x6", "3x5", "1x1", "12x2", "2x17"):
        monkeypatch.setenv("SST_RESIZE1_TILE", tile)
        assert torch.equal(rescale_to(x, rows, size), a) and torch.equal(rescale_to(x, rows, size, quantise=False), raw), tile
    monkeypatch.delenv("SST_RESIZE1_TILE")
    # the forms: a new tensor (the input untouched), out=; out is x raises; a non-contiguous input is read as it is indexed; rows on
    # the host are checked and uploaded
    keep = x.clone()
    o = torch.full((6, 3, *size), 7.0, device="cuda")
    assert rescale_to(x, rows, size, out=o) is o and torch.equal(o, a) and torch.equal(x, keep)
    sq = torch.zeros(6, 3, H, W, device="cuda")
    with pytest.raises(ValueError, match="out must not be x"):
        rescale_to(sq, rows, (H, W), out=sq)
    wide = torch.zeros(6, 3, H, 80, device="cuda")
    wide[..., :W] = x
    assert torch.equal(rescale_to(wide[..., :W], rows, size), a)
    with pytest.raises(ValueError, match="out must be contiguous fp32"):
        rescale_to(x, rows, size, out=torch.zeros(6, 3, 12, 20, device="cuda")[..., :17])
    with pytest.raises(ValueError, match="out must be contiguous fp32"):
        rescale_to(x, rows, size, out=torch.zeros(6, 3, 12, 18, device="cuda"))
    with pytest.raises(ValueError, match="deg must be contiguous int32"):
        rescale_to(x, rows[:4], size)
    with pytest.raises(ValueError, match="x must be fp32"):
        rescale_to(x.double(), rows, size)
    for bad_size in ((51, 17), (12, 71), (3, 17), (12, 4), (0, 17), (12.5, 17), (12,)):
        with pytest.raises(ValueError, match="rescale_to: (the output size|size must be a pair)"):
            rescale_to(x, rows, bad_size)
    assert torch.equal(rescale_to(x, rows.cpu(), size), a)
    for hi, wi in ((up8(H) - 1, W), (H, 2 * W + 1), (0, W), (-1, -1)):
        bad = rows.cpu().clone()
        bad[2, 0], bad[2, 1] = hi, wi
        with pytest.raises(ValueError, match="row 2: the intermediate size"):
            rescale_to(x, bad, size)


def test_nan_conventions_touch_that_sample_only():
    from srganst.device_data import rescale_to
    (H, W), size = (36, 44), (9, 11)
    spec = [("frac", "bicubic", "area", 5.0, 0.0, 0, 1), ("max", "bilinear", "bicubic", 0.0, 0.01, 1, 2), (None, "area", "area", 0.0, 0.0, 0, 3)]
    x = _input(3, H, W).cuda()
    good = _rows(spec, H, W)
    clean = rescale_to(x, good.cuda(), size)
    assert bool(torch.isfinite(clean).all())
    f32 = lambda v: int(np.float32(v).view(np.int32))
    sized, every = (0, 1), (0, 1, 2)
    cases = [(0, 0, sized), (1, 0, sized), (0, H, (2,)), (1, W, (2,)),                          # exactly one of hi, wi is zero
             (0, -3, every), (1, -3, every), (0, up8(H) - 1, sized), (1, up8(W) - 1, sized), (0, 2 * H + 1, sized), (1, 2 * W + 1, sized),
             (0, 1 << 30, sized), (0, -(1 << 31), sized),
             (6, 3, every), (6, 3 << 2, every), (6, 1 | 1 << 5, every), (6, 1 << 8, every), (6, -1, every), (6, -(1 << 31), every),
             (2, f32(-1e-3), every), (2, f32("nan"), every), (2, f32("-inf"), every), (3, f32(-1.0), every), (3, f32("nan"), every)]
    for word, value, victims in cases:
        for victim in victims:
            rows = good.clone()
            rows[victim, word] = value
            out = rescale_to(x, rows.cuda(), size)
            assert bool(torch.isnan(out[victim]).all()), (word, value, victim)
            for other in set(range(3)) - {victim}:
                assert torch.equal(out[other], clean[other]), (word, value, victim, other)
    # a NaN pixel reaches the outputs whose taps name it, and no other sample: keep + area, 4 x 4 blocks
    dirty = x.clone()
    dirty[2, 1, 17, 22] = float("nan")
    out = rescale_to(dirty, good.cuda(), size)
    mask = torch.zeros(3, 9, 11, dtype=torch.bool, device="cuda")
    mask[1, 4, 5] = True
    assert bool(torch.isnan(out[2][mask]).all()) and torch.equal(out[2][~mask], clean[2][~mask]) and torch.equal(out[:2], clean[:2])


def test_captured_launch_replayed_on_fresh_data_and_rows():
    from srganst.device_data import rescale_to
    (H, W), size = (36, 44), (9, 11)
    spec = [("frac", "bicubic", "bilinear", 10.0, 0.0, 0, 1), (None, "area", "area", 0.0, 0.0, 0, 2), ("max", "area", "area", 0.0, 0.02, 1, 3)]
    x, rows = _input(3, H, W).cuda(), _rows(spec, H, W).cuda()
    want = rescale_to(x, rows, size)
    buf, out = x.clone(), torch.zeros_like(want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one stream, one kernel node
        rescale_to(buf, rows, size, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    fresh = (_input(3, H, W).flip(0) * 0.9).contiguous().cuda()
    fresh_rows = _rows([("min", "bilinear", "bicubic", 0.0, 0.0, 0, 7), ("aniso", "area", "bicubic", 3.0, 0.0, 1, 8),
                        (None, "bilinear", "area", 4.0, 0.0, 0, 9)], H, W).cuda()
    buf.copy_(fresh), rows.copy_(fresh_rows)                                       # the graph reads both when it runs
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, rescale_to(fresh, fresh_rows, size))


# ---- the blur alone
@pytest.mark.parametrize("K", [7, 17])
def test_blur_then_the_stage_s_own_bicubic_is_the_fused_stage(K):
    """blur(gt, deg), then the first stage's bicubic tables on it (degrade with the no-blur sentinel), reproduces
    degrade(gt, deg, quantise=False) with noise off, bit for bit: the new path's blur is the fused one's.  A row without blur keeps
    the sample's bits; the noise word is not read; the forms agree."""
    from srganst.device_data import blur, degrade, degrade_rows
    H, W = 36, 44
    x = _input(4, H, W).cuda()
    keys = [(i, i + 1) for i in range(4)]
    deg = torch.from_numpy(degrade_rows([0.8, 3.0, 0.0, 1.7], [2.5, 0.6, 0.0, 1.7], [0.4, 2.0, 0.0, 0.0], [0.0] * 4, keys)).cuda()
    plain = torch.from_numpy(degrade_rows([0.0] * 4, [0.0] * 4, [0.0] * 4, [0.0] * 4, keys)).cuda()
    noisy = deg.clone()
    noisy[:, 3] = int(np.float32(0.1).view(np.int32))
    for scale in (4, 2):
        want = degrade(x, deg, scale, K, quantise=False)
        b = blur(x, deg, K)
        assert b.shape == x.shape and torch.equal(_bits(degrade(b, plain, scale, K, quantise=False)), _bits(want)), scale
    assert torch.equal(_bits(b[2]), _bits(x[2])) and not torch.equal(b[0], x[0]) and not torch.equal(b[3], x[3])
    assert torch.equal(blur(x, noisy, K), b)
    o = torch.full_like(x, 7.0)
    assert blur(x, deg, K, out=o) is o and torch.equal(o, b)
    assert torch.equal(blur(x[1:2].contiguous(), deg[1:2].contiguous(), K)[0], b[1])            # neither batch size nor position
    odd = x.clone()
    odd[2, 0, 0, 0], odd[2, 1, 5, 5] = float("nan"), -0.0
    assert torch.equal(_bits(blur(odd, deg, K)[2]), _bits(odd[2]))                               # the bits, whatever they are
    with pytest.raises(ValueError, match="out must not be x"):
        blur(x, deg, K, out=x)
    with pytest.raises(ValueError, match="deg must be contiguous int32"):
        blur(x, deg[:2], K)
    # a plane of more than one 32 x 32 tile in both directions, against the same tie-in
    big = _input(1, 70, 45).cuda()
    assert torch.equal(_bits(degrade(blur(big, deg[:1], K), plain[:1], 2, K, quantise=False)), _bits(degrade(big, deg[:1], 2, K, quantise=False)))


# ---- the loader
class _Counting:
    """_abi.lib() with every entry's calls counted."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def _second(ksize, **kw):
    from srganst.device_data import SecondOrder
    return SecondOrder(ksize=ksize, bank_size=24, sinc_bank_size=8, jpeg_quality=(20, 100), jpeg_chroma="444", jpeg_prob=0.7, **kw)


@pytest.mark.parametrize("scale, jpeg_prob, second", [(4, 0.0, False), (2, 0.5, False), (2, 0.5, True), (4, 0.5, True)])
def test_loader_with_the_first_stage_resize(scale, jpeg_prob, second, monkeypatch):
    """Two epochs over the small arena: lr is the public ops composed by hand - blur, rescale_to, jpeg on the loader's gt, then the
    second stage with its own resize - and degrade(gt, resize_rows=...); gt is the plain loader's; the last launch writes the bound
    buffer; an epoch repeats.  With the option off: the bits and the launches of the fused path, neither new entry called."""
    from srganst import _abi, device_data
    from srganst.device_data import Degradation, DeviceCropLoader, blur, degrade, jpeg, rescale_to, second_order
    S, B, K = 24, 2, 21
    o = S // scale
    _, arena, _, _ = _arena(S, scale)
    order = list(range(len(arena)))[::-1]
    kw = dict(blur_prob=0.8, noise_prob=0.8, jpeg_prob=jpeg_prob, jpeg_chroma="444", ksize=K)
    first, first_off = Degradation(**kw, resize_prob=(0.3, 0.4, 0.3)), Degradation(**kw)
    so = _second(21 if scale == 2 else 7, noise_prob=0.8, resize_prob=(0.3, 0.4, 0.3)) if second else None
    chroma2 = "444" if second else None
    on = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first, second=so)
    off = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=first_off, second=so)
    plain = DeviceCropLoader(arena, B, order, True, True, seed=2)
    gt_buf, lr_buf = torch.zeros(B, 3, S, S, device="cuda"), torch.zeros(B, 3, o, o, device="cuda")
    seen, kinds = [], np.zeros(3, np.int64)
    for epoch in range(2):
        deg, r1 = on.deg_draws(epoch), on.resize1_draws(epoch)
        assert np.array_equal(deg, off.deg_draws(epoch)) and off.resize1_draws(epoch) is None
        if second:
            rows2, bank = on.second_draws(epoch)
            bank_d, r2 = torch.from_numpy(bank).cuda(), on.resize_draws(epoch)
        if epoch == 1:
            on.bind(gt_buf, lr_buf)
        n = 0
        for (gt1, lr1), (gt0, _) in zip(on, plain):
            sel = order[n * B:(n + 1) * B]
            d = torch.from_numpy(np.ascontiguousarray(deg[sel])).cuda()
            rr = torch.from_numpy(np.ascontiguousarray(r1[sel])).cuda()
            kinds += [(rr[:, 0] > S).sum().item(), ((rr[:, 0] <= S) & (rr[:, 0] > 0)).sum().item(), (rr[:, 0] == 0).sum().item()]
            quiet = d.clone()
            quiet[:, 3] = 0                                                         # the blur launch with the noise word zeroed
            want = rescale_to(blur(gt0, quiet, K), rr, (o, o))
            if jpeg_prob:
                want = jpeg(want, d, "444")
            composed = degrade(gt0, d, scale, K, jpeg_chroma="444" if jpeg_prob else None, resize_rows=rr)
            assert torch.equal(composed, want)
            if second:
                rs = torch.from_numpy(np.ascontiguousarray(rows2[:, sel])).cuda()
                want = second_order(want, rs, bank_d, chroma2, resize_rows=torch.from_numpy(np.ascontiguousarray(r2[sel])).cuda())
            assert torch.equal(gt1, gt0) and torch.equal(lr1, want), (epoch, n)
            assert epoch == 0 or (lr1 is lr_buf and gt1 is gt_buf)
            assert float(lr1.min()) >= 0 and float(lr1.max()) <= 1 and float((lr1 * 255 - torch.round(lr1 * 255)).abs().max()) < 1e-3
            seen.append(lr1.clone())
            n += 1
        assert n == len(on) >= 3
    assert (kinds > 0).all(), kinds                                                # up, down and keep each ran on some sample
    on.bind(None, None)
    on.set_epoch(0)
    assert all(torch.equal(a, lr) for a, (_, lr) in zip(seen, on))
    # the launches, counted through _abi: the option on - the plain gather, sst_blur, sst_rescale_to per batch, no fused gather
    counting = _Counting(_abi.lib())
    monkeypatch.setattr(_abi, "lib", lambda: counting)
    on.set_epoch(0)
    nb = len(list(on))
    c = counting.calls
    assert c.get("sst_gather_crops") == nb and c.get("sst_blur") == nb and c.get("sst_rescale_to") == nb
    assert "sst_gather_crops_degraded" not in c and "sst_degrade" not in c and c.get("sst_jpeg", 0) == (nb if jpeg_prob else 0) + (nb if second else 0)
    # the option off: the bits of the loader built without the arguments (the parent's path) and neither new entry called
    counting.calls = {}
    parent = DeviceCropLoader(arena, B, order, True, True, seed=2, degradation=Degradation(**kw), second=so)
    off.set_epoch(0)
    got = [(gt.clone(), lr.clone()) for gt, lr in off]
    c = dict(counting.calls)
    assert "sst_blur" not in c and "sst_rescale_to" not in c and "sst_gather_crops" not in c
    assert c.get("sst_gather_crops_degraded") == nb and c.get("sst_rescale", 0) == (nb if second else 0)
    parent.set_epoch(0)
    plain.set_epoch(0)
    for (gt_a, lr_a), (gt_b, lr_b), (gt0, _) in zip(got, parent, plain):
        assert torch.equal(lr_a, lr_b) and torch.equal(gt_a, gt_b) and torch.equal(gt_a, gt0)
    if not second:                                                                  # and the fused stage is its stand-alone form
        off.set_epoch(0)
        deg = off.deg_draws(0)
        for n, (gt, lr) in enumerate(off):
            d = torch.from_numpy(np.ascontiguousarray(deg[order[n * B:(n + 1) * B]])).cuda()
            assert torch.equal(lr, degrade(gt, d, scale, K, jpeg_chroma="444" if jpeg_prob else None))


def test_loader_with_fixed_parameters_follows_the_restatement():
    """Degradation.fixed(resize=...) through the loader against the fp64 restatement, on the kernel's own blurred values."""
    from srganst.device_data import Degradation, DeviceCropLoader, blur, rescale_to
    S = 24
    _, arena, _, _ = _arena(S, 4)
    order = list(range(len(arena)))
    for resize in ((0.77, "bicubic", "area"), (1.5, "bilinear", "bicubic"), (0.15, "area", "bilinear")):
        first = Degradation.fixed(1.0, 2.0, 30.0, 3.0, key=5, resize=resize)
        on = DeviceCropLoader(arena, 4, order, degradation=first)
        deg, rr = on.deg_draws(0)[:4], on.resize1_draws(0)[:4]
        assert (rr[:, 0] == max(int(S * resize[0]), 3)).all() and np.array_equal(rr[:, 2], deg[:, 3])
        gt, lr = next(iter(on))
        b = blur(gt, torch.from_numpy(np.ascontiguousarray(deg)).cuda(), 21)
        raw = rescale_to(b, torch.from_numpy(np.ascontiguousarray(rr)).cuda(), (6, 6), quantise=False).cpu()
        ref = refs.rescale_to_reference(b.cpu().numpy(), rr, (6, 6), quantise=False)
        bound = refs.bound(rr, S, S, 6, 6, xmax=float(b.abs().max()))
        err = np.abs(raw.double().numpy() - ref).reshape(4, -1).max(1)
        assert (err <= bound).all(), (resize, err, bound)
        assert torch.equal(lr.cpu(), _grid(raw))


def test_warmup_trains_on_resized_batches(tmp_path, monkeypatch, capsys):
    from srganst.config import Config
    from srganst.loss import MSELoss
    from srganst.warmup import warmup
    from test_drivers_gpu import _Pairs
    monkeypatch.chdir(tmp_path)
    _, arena, _, _ = _arena(24, 4)
    cfg = Config()
    cfg.EXP.NAME, cfg.EXP.N_EPOCHS, cfg.EXP.SAVE_STATE = "resize1", 1, False
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    cfg.DATA.BATCH_SIZE, cfg.DATA.GT_IMAGE_SIZE, cfg.DATA.CROP_STEP = 2, 24, 8
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.LOG_TRAIN_PERIOD = 1
    cfg.DATA.ON_DEVICE_WHOLE_IMAGES = cfg.DATA.RANDOM_CROP = cfg.DATA.AUGMENT = cfg.DATA.DEGRADE = cfg.DATA.DEGRADE_RESIZE = True
    cfg.DATA.DEGRADE_JPEG_PROB = 0.5
    cfg.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": MSELoss()}
    cfg.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0}
    warmup(cfg, train_dataset=arena, test_dataset=_Pairs(), max_steps_per_epoch=3)
    out = capsys.readouterr().out
    assert out.count("[Data] DATA.DEGRADE_RESIZE: instead lr = ") == 1
    assert "(up, down, keep) = (0.2, 0.7, 0.1), scale in (0.15, 1.5), modes ('area', 'bilinear', 'bicubic')" in out
    losses = [float(v) for m in re.findall(r"\[G losses: \{([^}]*)\}", out) for v in re.findall(r": ([-+0-9.einfa]+)", m)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    assert os.path.exists("results/resize1/g_last.pth")


def test_validation_with_degrade_resize1(tmp_path, capsys):
    """Both validation paths, whole and tiled: the input is blur -> rescale_to at the scale s -> the later stages in their order; the
    head line names it; off: the numbers of before."""
    from torch.utils.data import DataLoader
    from srganst import kernels
    from srganst.config import Config
    from srganst.device_data import (Degradation, DeviceTestSet, blur, filter2d, filter_rows, jpeg, rescale, rescale_rows, rescale_to,
                                     resize1_size, resize_size)
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    cfg.EXP.NAME = "val"
    cfg.DATA.TEST_SR_IMAGES_DIR = str(tmp_path / "sr")
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB = 16, 1
    torch.manual_seed(3)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    ds = _TwoPairs()
    params, omega, s2, r1 = (0.6, 3.5, 30.0, 10.0), 1.5, 0.7, (0.4, "area", "bilinear")
    bank = torch.from_numpy(kernels.bank([kernels.sinc(21, omega)])).cuda()
    flt = torch.from_numpy(filter_rows([0], 0, 0, 0, [(0, 0)])).cuda()

    def first(hr, i, p, q=0):
        d = Degradation.fixed(*p, key=i, jpeg=q).draw(1)
        H, W = hr.shape[1:]
        rows = rescale_rows([(resize1_size(H, r1[0]), resize1_size(W, r1[0]))], r1[1:], p[3], 0.0, 0, [(i, 0)])
        return rescale_to(blur(hr[None].cuda(), d.cuda(), 21), torch.from_numpy(rows), (H // 4, W // 4)), d.cuda()

    def trip(t):
        h, w = t.shape[2:]
        rows = rescale_rows([(resize_size(h, s2), resize_size(w, s2))], ("bicubic", "bicubic"), 0, 0, 0, [(0, 0)])
        return rescale(t, torch.from_numpy(rows).cuda())
    want_alone = [first(hr, i, (0.0, 0.0, 0.0, 0.0))[0] for i, (hr, _) in enumerate(ds)]
    want_all = []
    for i, (hr, _) in enumerate(ds):
        lr, d = first(hr, i, params, 40)
        want_all.append(jpeg(filter2d(trip(lr), flt, bank), d, "420"))
    ref = refs.rescale_to_reference(ds[0][0][None].numpy(), rescale_rows([(51, 44)], r1[1:], 0, 0, 0, [(0, 0)]), (32, 28))
    assert np.abs(255 * (want_alone[0].cpu().double().numpy() - ref)).max() <= 1.0 + 1e-3
    fed = []
    hook = G.register_forward_pre_hook(lambda mod, args: fed.append(args[0].clone()))
    metrics_file = os.path.join(cfg.DATA.TEST_SR_IMAGES_DIR, "val", "_metrics.txt")
    results = {}
    for on_device in (False, True):
        loader = DeviceTestSet.from_dataset(ds, "cuda") if on_device else DataLoader(ds, batch_size=1, shuffle=False)
        for tile in (0, 24):
            plain = _validate(G, loader, cfg, on_device=on_device, tile=tile)
            capsys.readouterr()
            fed.clear()
            alone = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade_resize1=r1)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = "LR = resize1(GT): first-stage resize at scale 0.4 (area, then bilinear to the LR size) | "
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:                                # (tiled: the generator sees windows of the same input)
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_alone))
            fed.clear()
            every = _validate(G, loader, cfg, save_metrics=True, on_device=on_device, tile=tile, degrade=params, degrade_jpeg=40,
                              degrade_sinc=omega, degrade_resize=s2, degrade_resize1=r1)
            line, file = capsys.readouterr().out, open(metrics_file).read()
            head = ("LR = degrade(GT): sigma 0.6 / 3.5, theta 30 deg, noise 10, first-stage resize at scale 0.4 (area, then bilinear to the "
                    "LR size), resize round trip at scale 0.7 (bicubic), sinc cutoff 1.5, JPEG quality 40 (420) | ")
            assert line.startswith("[Test] | " + head + "PSNR: ") and file.startswith(head + "\n0.png | PSNR: ")
            if not tile:
                assert len(fed) == 2 and all(torch.equal(a, b) for a, b in zip(fed, want_all))
            _validate(G, loader, cfg, on_device=on_device, tile=tile, degrade_jpeg=40, degrade_resize1=r1)
            assert capsys.readouterr().out.startswith("[Test] | LR = jpeg(resize1(GT)): first-stage resize at scale 0.4 (area, then bilinear "
                                                      "to the LR size), JPEG quality 40 (420) | PSNR: ")
            cfg.DATA.VALIDATE_DEGRADE_RESIZE1 = r1
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == alone
            cfg.DATA.VALIDATE_DEGRADE_RESIZE1 = None
            assert _validate(G, loader, cfg, on_device=on_device, tile=tile) == plain
            assert len({plain, alone, every}) == 3 and all(math.isfinite(v) for v in alone + every)
            results[on_device, tile] = (alone, every)
    hook.remove()
    for tile in (0, 24):                                 # the host and the device metric paths agree
        for a, b in zip(results[False, tile], results[True, tile]):
            assert all(abs(u - v) <= 1e-6 * abs(u) for u, v in zip(a, b))
    for on_device in (False, True):                     # the tiled forward is the whole-image forward
        for a, b in zip(results[on_device, 0], results[on_device, 24]):
            assert all(abs(u - v) <= 1e-3 * abs(u) for u, v in zip(a, b))
