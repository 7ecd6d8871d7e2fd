"""GPU: the N-split 3x3 conv kernel (csrc/conv_nsplit.hip, conv_ns_kernel<S, TW>, entry sst_conv_ns_fwd) held to plain torch fp64 on the
CPU at all six template instances (stride 1 / 2 x tile width 8 / 4 / 2) and in every form it has: the NHWC store with bias, with the
input affine + LeakyReLU applied while staging and the BatchNorm statistics, the stride-1 data-gradient with the backward partials,
per-pass coefficient groups and the PixelShuffle store.

Rules:
  integer data                 x, w, bias, dy, saved y in [-3, 3], scales in {0.5, 1, 2}, non-zero integer shifts, slope 0.25: `exact`
                               asserts on the CPU that every partial sum stays below 2^24 in its unit, so fp32 sums are exact in any
                               order and y, g, cnt, stats[:, 0] and the three partial columns, per tile, must equal fp64 bit for bit
                               (the indexing test: a wrong tile, row wrap, group row, channel block or ring slot shows here).  M2 is
                               not exact (mean = s1 / nvalid): it is held to the random-data rule.
  random data                  norm-wise |hip - fp64| / |fp64| < TOL = 2e-5 (tests/test_kernels_gpu.py), and elementwise
                               |hip - fp64| <= k 2^-24 terms with terms = conv(|xin|, |w|) + |bias| in fp64 and k = 9 Cin + 8: an fp32 FMA
                               chain of 9 Cin terms in any association is within 9 Cin roundings of the sum of magnitudes, the other 8
                               cover the affine FMA, the slope multiply and the bias add.  The inputs are fp32 values, so the sign of
                               every fused z = y * scale + shift is the fp64 sign and no activation branch is undecided.
  statistics                   bn_finalize's mean within 1e-4 and rstd within 2e-5 (tests/test_conv_pipe_gpu.py), column totals of the
                               partials within 1e-4, per-tile sums / M2 / partials within TOL
Everything is compared with fp64 on the CPU; only test_against_the_k_split_kernel compares two kernels.  Every output the ops wrappers
allocate sits between sentinel-filled guard bands (glue_refs.Guarded), checked after each group of launches; a pixel the kernel never
stores keeps the sentinel and fails the comparison.  Each case first establishes its route: sst_conv_ns_supported gives the tile width,
sst_conv_pipe_stat_tiles the tile count, and the launch registers in ops.TRACE under conv_ns_kernel<S, TW>.

Which branch a case reaches.  All instance cases are (B, H, W) at Cin = 128, Cout = 256: two input-channel blocks (ncb = 2: the
`same_tile` reload `boffs += CB * 4` and the weight pointer step), two groups of four output-channel blocks (g_ > 0: `qq / n_mt`, the
weight block of group 1, stats rows written by both groups), Ho % TH != 0 (tiles straddle images: the row wrap of stage_load, `cross`
of lane_base), a partial last tile row (`rr < R`, nvalid), tiles_x >= 2 (ox0 != 0) and more units than the grid (768 workgroups at
stride 1, 512 at stride 2: the unit -> unit walk with the next unit's patch and weights in flight, workgroups that end early).
  <1, 8>  (103, 10, 16)   516 tiles, 1032 units, last tile row 2 of 4
  <1, 4>  (115, 12, 12)   519 tiles, 1038 units, last tile row 4 of 8
  <1, 2>  (545, 5, 6)     513 tiles, 1026 units, last tile row 5 of 16; Ho = 5: a tile crosses three image boundaries (NB = 3)
  <2, 8>  (171, 12, 32)   514 tiles, 1028 units, last tile row 2 of 4
  <2, 4>  (137, 20, 24)   516 tiles, 1032 units, last tile row 2 of 8
  <2, 2>  (545, 10, 12)   513 tiles, 1026 units, last tile row 5 of 16; NB = 3
  data-gradient (stride 1) the 256 -> 128 launch of the same layer at (207, 10, 16), (231, 12, 12), (1092, 5, 6): ncb = 4, one group,
                          1036 / 1041 / 1026 units > 768, last tile row 2 of 4 / 4 of 8 / 4 of 16; epi_scale / epi_shift given,
                          absent (slope from the device), epi_act = 0
  groups                  <1, 8> at (104, 10, 16) in passes of 26 images (4 rows of coefficients: `s.gin`), its data-gradient at
                          (208, 10, 16) in passes of 52 (`ge`), <2, 4> at (140, 20, 24) in passes of 20 (7 rows); a pass of 13 images
                          of <1, 8> does not end on a tile boundary and is refused
  PixelShuffle store      Cin = 64 (ncb = 1), Cout = 256, bias, PReLU on the input: <1, 4> at (69, 10, 12) 522 units, <1, 2> at
                          (273, 5, 6) 516 units, <1, 4> at (103, 10, 12) 774 units > 768 (the store after a unit -> unit step)
  against K-split         <1, 4> and <2, 4> with ops.CONV_NS off: same tiling (cnt bit-equal, stats of the same shape)

Worst elementwise ratio |hip - fp64| / (2^-24 terms) seen on the MI355X, plain / affine (bound k = 9 * 128 + 8 = 1160):
  <1, 8> 5.34 / 6.74   <1, 4> 6.31 / 6.71   <1, 2> 6.05 / 6.69   <2, 8> 5.34 / 6.33   <2, 4> 5.53 / 6.50   <2, 2> 5.72 / 7.11
  groups: <1, 8> 6.27 / 6.89, <2, 4> 5.77 / 8.66;  data-gradient (k = 9 * 256 + 8 = 2312): <1, 8> 6.22, <1, 4> 6.31, <1, 2> 5.49, groups 6.34;
  shuffle store (k = 9 * 64 + 8 = 584): 7.53, 5.85, 6.93.  Norm-wise: y, g and the per-tile partials 2e-7 .. 9e-7, the
  statistics below 4e-7, the column totals up to 1.2e-6.
k is the worst case of the chain (every rounding in the same direction); on random data the roundings mostly cancel, hence single digits.
Run with -s for the error tables."""
import functools

import pytest
import torch
import torch.nn.functional as F

import glue_refs as G
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
CIN, COUT = 128, 256
GRID = {1: 3 * 256, 2: 2 * 256}                                  # sst_conv_ns_fwd: workgroups per CU x CUs
THRESHOLD = {0: 1024, 1: 512}                                    # ns_plan: units below which the shape is not taken, by out_mode

# (S, TW) -> (B, H, W)
INSTANCES = {(1, 8): (103, 10, 16), (1, 4): (115, 12, 12), (1, 2): (545, 5, 6),
             (2, 8): (171, 12, 32), (2, 4): (137, 20, 24), (2, 2): (545, 10, 12)}
TABLE = {(1, 8): (1030, 516, 1032, 2), (1, 4): (1380, 519, 1038, 4), (1, 2): (2725, 513, 1026, 5),          # R, n_mt, units, last rows
         (2, 8): (1026, 514, 1028, 2), (2, 4): (1370, 516, 1032, 2), (2, 2): (2725, 513, 1026, 5)}
DGRAD = {(1, 8): (207, 10, 16), (1, 4): (231, 12, 12), (1, 2): (1092, 5, 6)}                               # the 256 -> 128 launch
GROUPS_FWD = {(1, 8): ((104, 10, 16), 26), (2, 4): ((140, 20, 24), 20)}
GROUPS_DGRAD = {(1, 8): ((208, 10, 16), 52)}
SHUFFLE = [(4, (69, 10, 12)), (2, (273, 5, 6)), (4, (103, 10, 12))]                                     # (TW, (B, H, W)) at 64 -> 256
IDS = lambda k: f"s{k[0]}_tw{k[1]}"


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def dev(t):
    return None if t is None else t.detach().to(torch.float32).contiguous().cuda()


def plan(B, H, W, s):
    """ns_plan / pipe_plan's tiling, restated: (TW, TH, Ho, Wo, R, tiles_x, n_mt, rows of the last tile row)."""
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    tw = 8 if Wo % 8 == 0 and Ho >= 3 else 4 if Wo % 4 == 0 and Ho >= 7 else 2 if Wo % 2 == 0 and Ho >= 5 else 0
    th, R = 32 // tw, B * Ho
    ty = (R + th - 1) // th
    return tw, th, Ho, Wo, R, Wo // tw, (Wo // tw) * ty, R - (ty - 1) * th


def route(ops, monkeypatch, shape, cin, cout, s, tw, out_mode=0):
    """Establishes that the built library sends the shape to conv_ns_kernel<s, tw> with the tile count the case was chosen for, and
    switches the launch trace on; -> (plan, kernel name)."""
    from srganst import _abi
    L = _abi.lib()
    pl = plan(*shape, s)
    assert pl[0] == tw
    assert L.sst_conv_ns_supported(*shape, cin, cout, 3, s, out_mode) == tw, (shape, cin, cout, s, out_mode)
    assert L.sst_conv_pipe_stat_tiles(*shape, cin, cout, 3, s) == pl[6], (shape, cin, cout, s)
    assert pl[6] * (cout // 128) >= THRESHOLD[out_mode]
    monkeypatch.setattr(ops, "TRACE", {})
    return pl, f"conv_ns_kernel<{s}, {tw}>"


def traced(ops, name, launches):
    assert set(ops.TRACE) == {name} and len(ops.TRACE[name]) == launches, {k: len(v) for k, v in ops.TRACE.items()}


def exact(bound, unit):
    """`bound`: the largest sum of magnitudes a chain can reach, all of whose terms are multiples of `unit` (a power of two): below
    2^24 unit every fp32 partial sum is exact whatever the order."""
    assert float(bound) / unit < 2 ** 24, f"sums up to {float(bound)} in units of {unit} leave the exact range of fp32"


def same(name, hip, ref64):
    hip = hip.detach().cpu()
    assert hip.dtype == torch.float32 and tuple(hip.shape) == tuple(ref64.shape), f"{name}: shape {tuple(hip.shape)} / {tuple(ref64.shape)}"
    if not torch.equal(hip.double(), ref64):
        bad = (hip.double() != ref64).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {ref64.numel()} elements differ from fp64, first at {bad[0].tolist()}: "
                             f"hip {hip[tuple(bad[0])].item()} ref {ref64[tuple(bad[0])].item()}")


def close(name, hip, ref64, report, tol=TOL):
    e = rel_err(hip.detach().cpu(), ref64)
    report.append((name, e, float("nan")))
    assert e < tol, f"{name}: |hip - fp64| / |fp64| = {e:.3e} >= {tol}"


def elementwise(name, hip, ref64, terms64, k, ratios):
    ratios.append((name, G.assert_elementwise(name, hip, ref64, terms64, k), k))


def show(title, report, ratios):
    G.print_report(title, report)
    for name, worst, k in ratios:
        print(f"  elementwise {name:30s} worst |hip - fp64| / (2^-24 terms) = {worst:8.2f}   (bound k = {k})")


# ================================================================================================ references (fp64, CPU)
def tiles_of(t, tw):
    """t [B, Ho, Wo, C] -> ([n_mt, 32, C] with the pixels of tile mt = ty * tiles_x + tx of the tall image [B Ho, Wo], rows past the
    end zero; valid [n_mt, 32])."""
    B, Ho, Wo, C = t.shape
    th, R = 32 // tw, B * Ho
    ty, tx = (R + th - 1) // th, Wo // tw
    tall = torch.zeros(ty * th, Wo, C, dtype=t.dtype)
    tall[:R] = t.reshape(R, Wo, C)
    v = tall.view(ty, th, tx, tw, C).permute(0, 2, 1, 3, 4).reshape(ty * tx, th * tw, C)
    ok = (torch.arange(ty * th) < R).view(ty, th, 1, 1).expand(ty, th, tx, tw).permute(0, 2, 1, 3).reshape(ty * tx, th * tw)
    return v, ok


def tile_stats(t, tw):
    """-> (sum [n_mt, C], M2 about the tile's own mean [n_mt, C], cnt [n_mt])."""
    v, ok = tiles_of(t, tw)
    cnt = ok.sum(1).to(t.dtype)
    s = v.sum(1)
    d = (v - (s / cnt.unsqueeze(1)).unsqueeze(1)) * ok.unsqueeze(2)
    return s, (d * d).sum(1), cnt


def tile_sums(t, tw):
    return tiles_of(t, tw)[0].sum(1)


def rows_of(coef, B, grp):
    """Per-channel coefficients [C] or [B / grp, C] -> [B, C, 1, 1]: image b uses row b // grp."""
    c = coef.view(-1, coef.shape[-1])
    return c.repeat_interleave(grp if grp else B, 0).view(B, -1, 1, 1)


def draws(seed, integer):
    gen = torch.Generator().manual_seed(seed + (0 if integer else 7))
    if integer:
        val = lambda *s: torch.randint(-3, 4, s, generator=gen).double()
        wgt = lambda *s: val(*s)
        scale = lambda *s: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, s, generator=gen)]
        shift = lambda *s: torch.randint(1, 4, s, generator=gen).double() * (2 * torch.randint(0, 2, s, generator=gen).double() - 1)
    else:
        val = lambda *s: torch.randn(*s, generator=gen).float().double()
        wgt = lambda *s: (torch.randn(*s, generator=gen) / (9 * s[1]) ** 0.5).float().double()
        scale = lambda *s: (torch.rand(*s, generator=gen) + 0.5).float().double()
        shift = lambda *s: (torch.randn(*s, generator=gen) * 0.3 + 0.5).float().double()
    slope = 0.25 if integer else float(torch.tensor(0.2).float())
    return val, wgt, scale, shift, slope


@functools.lru_cache(maxsize=1)
def forward_data(shape, s, integer, grp=0, cin=CIN):
    """Data and fp64 references of the forward forms, tensors NHWC: y of the plain conv with bias (`a`) and of the conv of
    lrelu(x * scale + shift) without bias (`b`), the sums of magnitudes of both, the channel statistics of `b`."""
    B, H, W = shape
    val, wgt, scale, shift, slope = draws(1009 * B + 31 * H + W + s + grp, integer)
    rows = (B // grp,) if grp else ()
    d = dict(x=val(B, cin, H, W), w=wgt(COUT, cin, 3, 3), b=val(COUT), sc=scale(*rows, cin), sh=shift(*rows, cin), slope=slope)
    xin = F.leaky_relu(d["x"] * rows_of(d["sc"], B, grp) + rows_of(d["sh"], B, grp), slope)
    d["xin"] = xin
    d["ya"] = nhwc(F.conv2d(d["x"], d["w"], d["b"], s, 1))
    d["yb"] = nhwc(F.conv2d(xin, d["w"], None, s, 1))
    if integer:
        wsum = d["w"].abs().sum(dim=(1, 2, 3)).max()
        exact(d["x"].abs().max() * wsum + 3, 1.0)                                       # y (+ bias)
        exact(xin.abs().max() * wsum, 0.125)                                            # x * 0.5 + shift, times 0.25: eighths
        exact(32 * d["yb"].abs().max(), 0.125)                                          # a tile's sum of up to 32 pixels
    else:
        d["ta"] = nhwc(F.conv2d(d["x"].abs(), d["w"].abs(), d["b"].abs(), s, 1))
        d["tb"] = nhwc(F.conv2d(xin.abs(), d["w"].abs(), None, s, 1))
    d["mean"] = d["yb"].mean(dim=(0, 1, 2))
    d["rstd"] = 1 / torch.sqrt(d["yb"].var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    return d


def check_forward(ops, monkeypatch, key, shape, integer, grp=0):
    s, tw = key
    B, H, W = shape
    (_, th, Ho, Wo, R, tiles_x, n_mt, last), name = route(ops, monkeypatch, shape, CIN, COUT, s, tw)
    d = forward_data(shape, s, integer, grp)
    report, ratios = [], []
    cmp = same if integer else (lambda n, h, r: close(n, h, r, report))
    tag = f"<{s}, {tw}> {shape}" + (f" grp {grp}" if grp else "")
    xd, wp = dev(nhwc(d["x"])), ops.pack_conv(dev(d["w"]))
    gd = G.Guarded()
    with gd.patch(ops):                                                                 # (a) plain, with bias
        ya = ops.conv_fwd(xd, wp, COUT, 3, s, bias=dev(d["b"]))[0]
    traced(ops, name, 1)
    cmp(f"y plain {tag}", ya, d["ya"])
    if not integer:
        elementwise(f"y plain {tag}", ya, d["ya"], d["ta"], 9 * CIN + 8, ratios)
    kw = dict(in_scale=dev(d["sc"]), in_shift=dev(d["sh"]), in_act=ops.ACT_SLOPE, want_stats=True, grp=grp)
    with gd.patch(ops):                                                                 # (b) affine + LeakyReLU while staging, statistics
        yb, _, st, cnt = ops.conv_fwd(xd, wp, COUT, 3, s, in_slope_const=d["slope"], **kw)
        yb2, _, st2, cnt2 = ops.conv_fwd(xd, wp, COUT, 3, s, in_slope_const=d["slope"], **kw)
        yc, _, stc, cntc = ops.conv_fwd(xd, wp, COUT, 3, s, in_slope=dev(torch.tensor([d["slope"]])), in_slope_const=0.0, **kw)
        gamma, beta = torch.ones(COUT, device="cuda"), torch.zeros(COUT, device="cuda")
        mean, rstd = ops.bn_finalize(st, cnt, gamma, beta)[:2]
    traced(ops, name, 4)
    s1, m2, n = tile_stats(d["yb"], tw)
    want_cnt = torch.full((n_mt,), float(th * tw), dtype=torch.float64)
    want_cnt[n_mt - tiles_x:] = last * tw
    assert torch.equal(n, want_cnt)
    for what, y_, st_, cnt_ in (("slope const", yb, st, cnt), ("slope tensor", yc, stc, cntc)):
        cmp(f"y affine {what} {tag}", y_, d["yb"])
        assert tuple(st_.shape) == (n_mt, 2, COUT) and tuple(cnt_.shape) == (n_mt,)
        assert float(cnt_.sum()) == B * Ho * Wo
        same(f"cnt {what} {tag}", cnt_, want_cnt)
        cmp(f"tile_sum {what} {tag}", st_[:, 0], s1)
        close(f"tile_M2 {what} {tag}", st_[:, 1], m2, report)
    if not integer:
        elementwise(f"y affine {tag}", yb, d["yb"], d["tb"], 9 * CIN + 8, ratios)
    close(f"mean {tag}", mean, d["mean"], report, 1e-4)
    close(f"rstd {tag}", rstd, d["rstd"], report, 2e-5)
    assert torch.equal(yb, yb2) and torch.equal(st, st2) and torch.equal(cnt, cnt2), f"second launch differs ({tag})"
    assert torch.equal(yb, yc) and torch.equal(st, stc), f"the slope from the device changes the result ({tag})"
    show(f"conv_ns forward {tag} {'integers' if integer else 'random'}", report, ratios)


@functools.lru_cache(maxsize=1)
def dgrad_data(shape, integer, grp=0):
    """The data-gradient of the CIN -> COUT layer (a COUT -> CIN launch) and what its epilogue sums, NHWC."""
    B, H, W = shape
    val, wgt, scale, shift, slope = draws(2003 * B + 37 * H + W + grp, integer)
    rows = (B // grp,) if grp else ()
    d = dict(w=wgt(COUT, CIN, 3, 3), dy=val(B, COUT, H, W), y=nhwc(val(B, CIN, H, W)), sc=scale(*rows, CIN), sh=shift(*rows, CIN),
             slope=slope)
    if not integer:
        d["w"] = (d["w"] * (CIN / COUT) ** 0.5).float().double()                        # 9 COUT terms per output
    d["g"] = nhwc(torch.nn.grad.conv2d_input((B, CIN, H, W), d["w"], d["dy"], 1, 1))
    if integer:
        gmax = d["g"].abs().max()
        exact(d["dy"].abs().max() * d["w"].abs().sum(dim=(0, 2, 3)).max(), 1.0)         # g
        exact(32 * gmax * 9, 0.25)                                                      # |y| <= 3, |z| <= 3 * 2 + 3; g * slope: quarters
    else:
        d["tg"] = nhwc(torch.nn.grad.conv2d_input((B, CIN, H, W), d["w"].abs(), d["dy"].abs(), 1, 1))
    return d


def check_dgrad(ops, monkeypatch, tw, shape, integer, grp=0):
    B, H, W = shape
    (_, th, Ho, Wo, R, tiles_x, n_mt, last), name = route(ops, monkeypatch, shape, COUT, CIN, 1, tw)
    assert n_mt > GRID[1]
    d = dgrad_data(shape, integer, grp)
    report, ratios = [], []
    cmp = same if integer else (lambda n, h, r: close(n, h, r, report))
    tag = f"<1, {tw}> {shape}" + (f" grp {grp}" if grp else "")
    dyd, wd, yd = dev(nhwc(d["dy"])), ops.pack_conv(dev(d["w"]), 1), dev(d["y"])
    sc, sh = rows_of(d["sc"], B, grp).view(B, 1, 1, CIN), rows_of(d["sh"], B, grp).view(B, 1, 1, CIN)
    variants = [("scale+shift", dict(epi_scale=dev(d["sc"]), epi_shift=dev(d["sh"]), epi_slope_const=d["slope"], epi_act=1, grp=grp),
                 (sc, sh, 1))]
    if not grp:
        variants += [("no affine", dict(epi_slope=dev(torch.tensor([d["slope"]])), epi_slope_const=0.0, epi_act=1), (None, None, 1)),
                     ("no act", dict(epi_slope_const=d["slope"], epi_act=0), (None, None, 0))]
    gd = G.Guarded()
    for i, (what, kw, (rs, rh, act)) in enumerate(variants):
        with gd.patch(ops):
            g, part = ops.conv_dgrad_bwdstats(dyd, wd, CIN, 3, yd, **kw)
            g2, part2 = ops.conv_dgrad_bwdstats(dyd, wd, CIN, 3, yd, **kw)
        traced(ops, name, 2 * i + 2)
        cmp(f"g {what} {tag}", g, d["g"])
        if not integer:
            elementwise(f"g {what} {tag}", g, d["g"], d["tg"], 9 * COUT + 8, ratios)
        gz, gm = G.bwd_gz(d["g"], d["y"], rs, rh, d["slope"], act)
        want = torch.stack([tile_sums(gz, tw), tile_sums(gz * d["y"], tw), tile_sums(gm, tw)], 1)
        assert tuple(part.shape) == (n_mt, 3, CIN)
        for j, col in enumerate(("sum_gz", "sum_gz_y", "sum_g_minz0")):
            if act or j < 2:
                cmp(f"part_{col} {what} {tag}", part[:, j], want[:, j])
                close(f"total_{col} {what} {tag}", part.double().sum(0)[j], want.sum(0)[j], report, 1e-4)
            else:
                same(f"part_{col} {what} {tag}", part[:, j], want[:, j])                # epi_act = 0: exactly zero
        assert torch.equal(g, g2) and torch.equal(part, part2), f"second launch differs ({what}, {tag})"
    show(f"conv_ns data-gradient {tag} {'integers' if integer else 'random'}", report, ratios)


# ================================================================================================ 0. the case table
def test_case_table_reaches_the_branches():
    """The conditions the cases were chosen for, restated from ns_plan and the kernel: if either changes, re-choose the cases."""
    for (s, tw), shape in INSTANCES.items():
        ptw, th, Ho, Wo, R, tiles_x, n_mt, last = plan(*shape, s)
        assert (ptw, R, n_mt, n_mt * (COUT // 128), last) == (tw,) + TABLE[(s, tw)]
        assert Ho % th and last < th and tiles_x >= 2 and n_mt * (COUT // 128) > GRID[s] and CIN // 64 == 2
        crossings = max((ty * th % Ho + th - 1) // Ho for ty in range(R // th))
        assert crossings == (3 if tw == 2 else 1)
    for tw, shape in DGRAD.items():
        ptw, th, Ho, _, R, tiles_x, n_mt, last = plan(*shape, 1)
        assert ptw == tw[1] and n_mt >= 1024 and Ho % th and last < th
    for table in (GROUPS_FWD, GROUPS_DGRAD):
        for (s, tw), (shape, grp) in table.items():
            ptw, th, Ho, _, _, _, n_mt, _ = plan(*shape, s)
            assert ptw == tw and shape[0] % grp == 0 and (grp * Ho) % th == 0 and Ho % th and n_mt >= 1024 // (2 if table is GROUPS_FWD else 1)
    for (tw, shape), units in zip(SHUFFLE, (522, 516, 774)):
        assert plan(*shape, 1)[0] == tw and plan(*shape, 1)[6] * 2 == units
    assert SHUFFLE[2][0] in (8, 4) and 774 > GRID[1]


# ================================================================================================ 1. forward, NHWC
@pytest.mark.parametrize("key", list(INSTANCES), ids=IDS)
def test_forward_exact_on_integers(ops, monkeypatch, key):
    """Plain with bias; affine + LeakyReLU while staging (slope as a constant and from the device) with statistics: y, cnt and the
    per-tile sums bit-equal to fp64, the padding exactly zero (every shift is at least 1 in magnitude)."""
    check_forward(ops, monkeypatch, key, INSTANCES[key], integer=True)


@pytest.mark.parametrize("key", list(INSTANCES), ids=IDS)
def test_forward_random_vs_fp64(ops, monkeypatch, key):
    check_forward(ops, monkeypatch, key, INSTANCES[key], integer=False)


# ================================================================================================ 2. stride-1 data-gradient + partials
@pytest.mark.parametrize("key", list(DGRAD), ids=IDS)
def test_dgrad_partials_exact_on_integers(ops, monkeypatch, key):
    """ops.conv_dgrad_bwdstats with mode-1 packed weights (ncb = 4): g and the three partial columns of every tile bit-equal to fp64,
    with epi_scale / epi_shift, without, and with epi_act = 0."""
    check_dgrad(ops, monkeypatch, key[1], DGRAD[key], integer=True)


@pytest.mark.parametrize("key", list(DGRAD), ids=IDS)
def test_dgrad_partials_random_vs_fp64(ops, monkeypatch, key):
    check_dgrad(ops, monkeypatch, key[1], DGRAD[key], integer=False)


# ================================================================================================ 3. coefficient groups
@pytest.mark.parametrize("integer", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("key", list(GROUPS_FWD), ids=IDS)
def test_forward_coefficient_groups(ops, monkeypatch, key, integer):
    """in_scale / in_shift [B / grp, Cin], a different row per pass, against fp64 with each pass's own coefficients."""
    shape, grp = GROUPS_FWD[key]
    check_forward(ops, monkeypatch, key, shape, integer, grp=grp)


@pytest.mark.parametrize("integer", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("key", list(GROUPS_DGRAD), ids=IDS)
def test_dgrad_coefficient_groups(ops, monkeypatch, key, integer):
    """epi_scale / epi_shift [B / grp, Cout of the launch]."""
    shape, grp = GROUPS_DGRAD[key]
    check_dgrad(ops, monkeypatch, key[1], shape, integer, grp=grp)


def test_groups_off_a_tile_boundary_are_refused(ops, monkeypatch):
    """<1, 8> at (104, 10, 16): passes of 13 images are 130 rows, not a multiple of TH = 4."""
    from srganst._abi import HipPathError
    z = lambda *s: torch.zeros(*s, device="cuda")
    shape, grp = (104, 10, 16), 13
    route(ops, monkeypatch, shape, CIN, COUT, 1, 8)
    assert shape[0] % grp == 0 and (grp * shape[1]) % 4
    with pytest.raises(HipPathError):
        ops.conv_fwd(z(*shape, CIN), ops.pack_conv(z(COUT, CIN, 3, 3)), COUT, 3, 1, in_scale=z(8, CIN), in_shift=z(8, CIN), in_act=ops.ACT_SLOPE, grp=grp)
    shape = (208, 10, 16)
    route(ops, monkeypatch, shape, COUT, CIN, 1, 8)
    with pytest.raises(HipPathError):
        ops.conv_dgrad_bwdstats(z(*shape, COUT), ops.pack_conv(z(COUT, CIN, 3, 3), 1), CIN, 3, z(*shape, CIN), epi_scale=z(16, CIN), epi_shift=z(16, CIN),
                                epi_act=1, grp=grp)
    torch.cuda.synchronize()
    assert not ops.TRACE


# ================================================================================================ 4. PixelShuffle store
@pytest.mark.parametrize("tw, shape", SHUFFLE, ids=lambda p: str(p).replace(" ", ""))
def test_shuffle_store(ops, monkeypatch, tw, shape):
    """64 -> 256 with bias and PReLU on the input, stored as PixelShuffle(2): against F.pixel_shuffle(F.conv2d(...)) in fp64, integers
    bit-equal, random data norm-wise and elementwise."""
    B, H, W = shape
    cin = 64
    _, name = route(ops, monkeypatch, shape, cin, COUT, 1, tw, out_mode=ops.OUT_SHUFFLE)
    launches = 0
    for integer in (True, False):
        val, wgt, _, _, slope = draws(B + H + W, integer)
        x, w, b = val(B, cin, H, W), wgt(COUT, cin, 3, 3), val(COUT)
        xin = F.leaky_relu(x, slope)
        ref = nhwc(F.pixel_shuffle(F.conv2d(xin, w, b, 1, 1), 2))
        if integer:
            exact(xin.abs().max() * w.abs().sum(dim=(1, 2, 3)).max() + 3, 0.25)
        gd = G.Guarded()
        with gd.patch(ops):
            kw = dict(bias=dev(b), in_slope=dev(torch.tensor([slope])), in_act=ops.ACT_SLOPE, out_mode=ops.OUT_SHUFFLE)
            y, _, st, cnt = ops.conv_fwd(dev(nhwc(x)), ops.pack_conv(dev(w)), COUT, 3, 1, **kw)
            y2 = ops.conv_fwd(dev(nhwc(x)), ops.pack_conv(dev(w)), COUT, 3, 1, **kw)[0]
        launches += 2
        traced(ops, name, launches)
        assert st is None and cnt is None and tuple(y.shape) == (B, 2 * H, 2 * W, COUT // 4)
        assert torch.equal(y, y2), f"second launch differs ({shape})"
        if integer:
            same(f"y shuffle {shape}", y, ref)
        else:
            report, ratios = [], []
            close(f"y shuffle {shape}", y, ref, report)
            terms = nhwc(F.pixel_shuffle(F.conv2d(xin.abs(), w.abs(), b.abs(), 1, 1), 2))
            elementwise(f"y shuffle {shape}", y, ref, terms, 9 * cin + 8, ratios)
            show(f"conv_ns shuffle store <1, {tw}> {shape}", report, ratios)


# ================================================================================================ 5. against the K-split kernel
@pytest.mark.parametrize("key", [(1, 4), (2, 4)], ids=IDS)
def test_against_the_k_split_kernel(ops, monkeypatch, key):
    """The same launch on conv_pipe_kernel (ops.CONV_NS off): y within 1e-5, cnt bit-equal, stats of the same shape - both kernels
    share the tiling, and the host sizes the statistics by it."""
    s, tw = key
    shape = INSTANCES[key]
    _, name = route(ops, monkeypatch, shape, CIN, COUT, s, tw)
    gen = torch.Generator().manual_seed(5 + s)
    x = torch.randn(*shape, CIN, generator=gen).cuda()
    wp = ops.pack_conv((torch.randn(COUT, CIN, 3, 3, generator=gen) / (9 * CIN) ** 0.5).cuda())
    sc, sh = (torch.rand(CIN, generator=gen) + 0.5).cuda(), (torch.randn(CIN, generator=gen) * 0.3).cuda()
    kw = dict(in_scale=sc, in_shift=sh, in_slope_const=0.2, in_act=ops.ACT_SLOPE, want_stats=True)
    gd = G.Guarded()
    with gd.patch(ops):
        y1, _, st1, cnt1 = ops.conv_fwd(x, wp, COUT, 3, s, **kw)
    traced(ops, name, 1)
    monkeypatch.setattr(ops, "CONV_NS", False)
    monkeypatch.setattr(ops, "TRACE", {})
    with gd.patch(ops):
        y0, _, st0, cnt0 = ops.conv_fwd(x, wp, COUT, 3, s, **kw)
    traced(ops, f"conv_pipe_kernel<{s}, {tw}, 0>", 1)
    assert rel_err(y1.cpu(), y0.cpu()) < 1e-5
    assert torch.equal(cnt1, cnt0) and st1.shape == st0.shape
    assert rel_err(st1[:, 0].cpu(), st0[:, 0].cpu()) < 1e-5


# ================================================================================================ 6. host refusals
def test_host_refusals():
    """sst_conv_ns_fwd refuses, before any launch: statistics or partials with the shuffle store, partials together with statistics, a
    shape below the threshold, in_scale without in_shift.  All buffers have the sizes an accepted call would need."""
    from srganst import _abi
    from srganst._abi import HipPathError, check, ptr, stream_ptr
    L = _abi.lib()
    gd = G.Guarded()
    z = lambda *s: gd.empty(*s, fill=0.0)

    def call(shape, cin, out_mode, in_scale=False, in_shift=False, stats=False, part=False):
        B, H, W = shape
        n_mt = plan(*shape, 1)[6]
        x, wp = z(B, H, W, cin), z(L.sst_conv_packed_floats(COUT, cin, 3))
        y = z(B, 2 * H, 2 * W, COUT // 4) if out_mode else z(B, H, W, COUT)
        st, cnt = (z(n_mt, 2, COUT), z(n_mt)) if stats else (None, None)
        ey, ep = (z(B, H, W, COUT), z(n_mt, 3, COUT)) if part else (None, None)
        rc = L.sst_conv_ns_fwd(ptr(x), ptr(wp), ptr(y), None, ptr(z(cin)) if in_scale else None, ptr(z(cin)) if in_shift else None, None,
                               0.2, 1, ptr(st), ptr(cnt), ptr(ey), None, None, None, 0.2, 1, ptr(ep), B, H, W, cin, COUT, 3, 1, out_mode, 0,
                               stream_ptr())
        check(rc, "sst_conv_ns_fwd")

    shuffle, nhwc_shape = SHUFFLE[0][1], INSTANCES[(1, 8)]
    assert L.sst_conv_ns_supported(*shuffle, 64, COUT, 3, 1, 1) and L.sst_conv_ns_supported(*nhwc_shape, CIN, COUT, 3, 1, 0)
    assert not L.sst_conv_ns_supported(4, 10, 16, CIN, COUT, 3, 1, 0)
    refused = [dict(shape=shuffle, cin=64, out_mode=1, stats=True), dict(shape=shuffle, cin=64, out_mode=1, part=True),
               dict(shape=nhwc_shape, cin=CIN, out_mode=0, stats=True, part=True), dict(shape=(4, 10, 16), cin=CIN, out_mode=0),
               dict(shape=nhwc_shape, cin=CIN, out_mode=0, in_scale=True), dict(shape=nhwc_shape, cin=CIN, out_mode=0, in_shift=True)]
    for kw in refused:
        with pytest.raises(HipPathError):
            call(**kw)
    for buf, n in gd.bufs:                                                               # nothing ran: every buffer still holds its zeros
        assert not bool(buf[G.GUARD:G.GUARD + n].any())
    gd.check()
    call(shape=nhwc_shape, cin=CIN, out_mode=0, in_scale=True, in_shift=True, stats=True)  # and the library still takes a good call
    gd.check()
