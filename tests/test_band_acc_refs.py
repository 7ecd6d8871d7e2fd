"""CPU: tests/band_acc_refs.py - the restatements tests/test_conv_band_acc_fp64_gpu.py holds the accumulator-mode band conv to - held
themselves to F.batch_norm, F.conv2d and autograd in fp64, so a wrong formula there cannot pass a wrong kernel; plus the host mirror of
the band selection, the exactness of the integer-data cases and the share of pinned activation signs."""
import pytest
import torch
import torch.nn.functional as F

import band_acc_refs as R
import glue_refs as G

D = torch.float64
TIGHT = 1e-11


def close(name, a, b, tol=TIGHT):
    a, b = a.detach().double(), b.detach().double()
    e = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert e < tol, f"{name}: {e:.3e}"


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("case", list(R.CASES))
def test_band_rows_mirror_reproduces_the_case_table(case):
    (B, H, W), want, route = R.CASES[case]
    assert R.band_rows(H, W, int(want) if want else 3) == route
    nb, rr, patch = route
    assert nb * 16 == rr * W and H % rr == 0 and patch == (rr + 2) * (W + 2)


def test_band_rows_mirror_paths():
    assert [R.late_reduction(*R.CASES[c][2][::2]) for c in "abcdefgh"] == [True, False, True, True, False, False, False, False]
    assert R.band_rows(6, 24, 3) == (3, 2, 104) and R.band_rows(6, 24, 9) == (9, 6, 208)
    for B, H, W in R.REFUSED_SHAPES:
        assert R.band_rows(H, W, 3) is None and R.band_rows(H, W, 9) is None
    assert R.band_rows(2, 72, 9) == (9, 2, 296)                       # W = 72 fits; W = 144 only fails the LDS limit
    assert 4 * 4 * 3 * 146 * R.PSTR > R.LDS_LIMIT
    assert R.band_rows(6, 4, 3) is None                               # W < 8
    assert len(R.CONFIGS) == 18 and max(B * H * W for (B, H, W), _, _ in R.CASES.values()) == 17 * 2 * 48


# ------------------------------------------------------------------------------------------------ restatements against F.* / autograd
@pytest.mark.parametrize("nrep", [1, 5, 16])
def test_forward_rows_and_finalize_are_batch_norm(nrep):
    gen = torch.Generator().manual_seed(3)
    B, H, W, C = 7, 2, 8, 64
    y = torch.randn(B, H, W, C, generator=gen, dtype=D) * 2 + 3
    gamma, beta = torch.rand(C, generator=gen, dtype=D) + 0.5, torch.randn(C, generator=gen, dtype=D)
    rm, rv = torch.randn(C, generator=gen, dtype=D), torch.rand(C, generator=gen, dtype=D) + 0.5
    acc, mag = R.fwd_acc_of(y, nrep)
    assert acc.shape == (nrep, C, 2) and bool((mag >= acc.abs() - 1e-9).all())
    for r in range(nrep):
        close(f"replica {r}", acc[r, :, 0], y[r::nrep].sum((0, 1, 2)))
        close(f"replica {r} squares", acc[r, :, 1], (y[r::nrep] ** 2).sum((0, 1, 2)))
    n = B * H * W
    f = R.fwd_finalize(acc, n, gamma, beta, rm, rv, D)
    rm_t, rv_t = rm.clone(), rv.clone()
    z = F.batch_norm(y.reshape(n, C), rm_t, rv_t, gamma, beta, True, R.MOMENTUM, R.EPS)
    close("affine", y.reshape(n, C) * f["scale"] + f["shift"], z)
    close("run_mean", f["run_mean"], rm_t)
    close("run_var", f["run_var"], rv_t)
    close("mean", f["mean"], y.mean((0, 1, 2)))
    close("rstd", f["rstd"], 1 / torch.sqrt(y.var((0, 1, 2), unbiased=False) + R.EPS))
    biased = (1 - R.MOMENTUM) * rv + R.MOMENTUM * y.var((0, 1, 2), unbiased=False)
    assert float(((f["run_var"] - biased).abs() / biased).min()) > 100 * R.K_RUNVAR * R.U24       # n - 1 is told from n


def test_convs_and_staged_inputs():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 8, 64, generator=gen, dtype=D, requires_grad=True)
    w = torch.randn(32, 64, 3, 3, generator=gen, dtype=D)
    up = torch.randn(2, 4, 8, 32, generator=gen, dtype=D)
    y = R.conv(x, w)
    close("conv", y, F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1))
    y.backward(up)
    close("dgrad", R.dgrad(up, w), x.grad)
    sc, sh = torch.rand(64, generator=gen, dtype=D) + 0.5, torch.randn(64, generator=gen, dtype=D)
    xd = x.detach()
    close("prelu", R.staged_fwd(xd, sc, sh, 0.2, True), F.leaky_relu(xd * sc + sh, 0.2))
    close("no act", R.staged_fwd(xd, sc, sh, 0.2, False), xd * sc + sh)
    close("plain", R.staged_fwd(xd, None, None, 0.2, True), F.leaky_relu(xd, 0.2))
    assert bool((R.conv_terms(xd, w) >= R.conv(xd, w).abs() - 1e-9).all())


@pytest.mark.parametrize("act", [0, 1])
def test_backward_rows_and_coefficients_are_autograd(act):
    gen = torch.Generator().manual_seed(5 + act)
    B, H, W, C, nrep = 6, 2, 8, 64, 4
    n = B * H * W
    y = torch.randn(B, H, W, C, generator=gen, dtype=D) + 0.5
    g = torch.randn(B, H, W, C, generator=gen, dtype=D)
    gamma, beta = torch.rand(C, generator=gen, dtype=D) + 0.5, torch.randn(C, generator=gen, dtype=D) * 0.3
    slope = torch.tensor([0.2], dtype=D)
    f = R.fwd_finalize(R.fwd_acc_of(y, nrep)[0], n, gamma, beta, None, None, D)
    acc, mag = R.bwd_acc_of(g, y, f["scale"], f["shift"], slope, act, nrep)
    assert acc.shape == (nrep, C, 4) and bool((acc[..., 3] == 0).all()) and bool((mag >= acc.abs() - 1e-9).all())
    co = R.bwd_finalize(acc, n, f["mean"], f["rstd"], gamma, D)
    dy = R.staged_bwd(g, y, f["scale"], f["shift"], slope, act, co)
    ag = G.chain_grads(y.reshape(n, C), g.reshape(n, C), gamma, beta, slope, act, D)
    close("dy", dy.reshape(n, C), ag["dy"], 1e-9)
    close("dgamma", co["dgamma"], ag["dgamma"], 1e-9)
    close("dbeta", co["dbeta"], ag["dbeta"], 1e-9)
    if act:
        close("dslope", co["dslope"], ag["dslope"], 1e-9)
    flipped = dict(co, cC=co["cC"] - 2 * co["cA"] * f["rstd"] * f["mean"] * (f["rstd"] * (R.totals(acc)[:, 1] - f["mean"] * R.totals(acc)[:, 0]) / n))
    assert float((R.staged_bwd(g, y, f["scale"], f["shift"], slope, act, flipped).reshape(n, C) - ag["dy"]).abs().max()) > 1e-4


@pytest.mark.parametrize("case", R.BLOCK_CASES)
def test_block_restated_is_block_autograd(case):
    (B, H, W), _, _ = R.CASES[case]
    p = R.block_params(11)
    gen = torch.Generator().manual_seed(12)
    h, up = torch.randn(B, H, W, 64, generator=gen, dtype=D), torch.randn(B, H, W, 64, generator=gen, dtype=D)
    a, r = R.block(h, p, up, D), R.block_restated(h, p, up, 5, D)
    for k in a:
        close(k, r[k], a[k], 1e-9)


# ------------------------------------------------------------------------------------------------ hand-written accumulators
@pytest.mark.parametrize("nrep", [1, 4, 5, 16])
def test_hand_written_forward_accumulators(nrep):
    n = 5 * 6 * 24
    hw = R.hand_fwd_acc(nrep, n, 21, False)
    acc = hw["acc"]
    close("totals", R.totals(acc)[:, 0], hw["yv"].sum(0))
    if nrep > 1:
        assert bool(((acc[..., 0] > 0).any(0) & (acc[..., 0] < 0).any(0)).all()), "every channel has partial sums of both signs"
        assert float((acc.abs().max(0).values / acc.abs().min(0).values.clamp_min(1e-300)).median()) > 3, "uneven split"
    f = R.fwd_finalize(acc, n, hw["gamma"], hw["beta"], None, None, D)
    close("mean", f["mean"], hw["yv"].mean(0), 1e-9)
    hi = R.hand_fwd_acc(nrep, n, 21, True)
    f = R.fwd_finalize(hi["acc"], n, hi["gamma"], hi["beta"], None, None, D)
    assert torch.equal(f["mean"], hi["mean"])
    # the kernel's own arithmetic: var = (float)(m2 / n), rstd = 1 / sqrtf(var + eps) - exactly the power of two
    t = R.totals(hi["acc"])
    var32 = ((t[:, 1] - t[:, 0] * (t[:, 0] / n)) / n).float()
    assert torch.equal((1 / torch.sqrt(var32 + torch.tensor(R.EPS, dtype=torch.float32))).double(), hi["rstd"])
    assert bool((hi["acc"] * 2 ** 27 == (hi["acc"] * 2 ** 27).round()).all()) and float(hi["acc"].abs().max()) < 2 ** 14


@pytest.mark.parametrize("act", [0, 1])
def test_hand_written_backward_accumulators(act):
    n, nrep = 3 * 2 * 48, 5
    hi = R.hand_bwd_acc(nrep, n, 31, True, act)
    assert bool((hi["acc"][..., 3] == 1e30).all())
    co = R.bwd_finalize(hi["acc"][..., :3], n, hi["mean"], hi["rstd"], hi["gamma"], D)
    for k in ("cA", "cB", "cC", "dgamma", "dbeta", "dslope"):
        assert bool((co[k] * 64 == (co[k] * 64).round()).all()) and float(co[k].abs().max()) < 2 ** 12, f"{k} is a small dyadic number"
        assert torch.equal(co[k].float().double(), co[k])
    hr = R.hand_bwd_acc(nrep, n, 31, False, act)
    assert bool(((hr["acc"][..., 0] > 0).any(0) & (hr["acc"][..., 0] < 0).any(0)).all())


# ------------------------------------------------------------------------------------------------ exactness of the integer cases
@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_integer_cases_stay_exact_in_fp32(config):
    """Every fp32 partial sum of the integer-data launches stays below 2^24 in its unit: the sums of magnitudes of the conv chains and of
    the band totals (plain sums are fp32 per band), and each term of the three backward sums (formed in fp32, summed in fp64)."""
    B, H, W, cout, nrep, n, rr = R.dims(config)
    d = R.fwd_data(config, True)
    x, x2, w, bias, slope = d["x"], d["x2"], d["w"], d["bias"], d["slope"]
    bands = lambda t: t.view(B, H // rr, rr * W, cout).sum(2).max()
    for act in (0, 1):                                                                      # producer
        y_mag = R.conv_terms(R.staged_fwd(x, None, None, slope, act), w, bias)
        R.exact("producer y", y_mag.max(), 0.25)
        R.exact("producer band total", bands(y_mag), 0.25)
    hw = R.hand_fwd_acc(nrep, n, 42, True)                                                   # consumer: scale, shift are dyadic
    f = R.exact_affine(hw)
    for k in ("scale", "shift"):
        assert bool((f[k] * 8 == (f[k] * 8).round()).all()) and float(f[k].abs().max()) <= 64
    for staged in (R.staged_fwd(x, f["scale"], f["shift"], slope, True), R.staged_fwd(x, f["scale"], f["shift"], slope, False),
                   R.staged_res(x, x2, f["scale"], f["shift"])):
        assert bool((staged * 32 == (staged * 32).round()).all())
        y_mag = R.conv_terms(staged, w, bias)
        R.exact("consumer y", y_mag.max(), 1 / 32)
        R.exact("consumer band total", bands(y_mag), 1 / 32)
    b = R.bwd_data(config, True)                                                             # backward producer
    out_mag = R.conv_terms(b["g"], b["wd"], None, b["res"], transposed=True)
    R.exact("dgrad out", out_mag.max(), 1.0)
    zmax = float((b["ysave"].abs() * b["esc"] + b["esh"].abs()).max())
    R.exact("backward terms", out_mag.max() * max(zmax, 3.0), 1 / 8)                          # formed in fp32, summed in fp64
    for act in (0, 1):                                                                      # backward stage
        hb = R.hand_bwd_acc(nrep, n, 43, True, act)
        co = R.bwd_finalize(hb["acc"][..., :3], n, hb["mean"], hb["rstd"], hb["gamma"], D)
        dy = R.staged_bwd(b["g"], b["y2"], b["isc"], b["ish"], slope, act, co)
        assert bool((dy * 256 == (dy * 256).round()).all()) and float(dy.abs().max()) < 2 ** 12
        out_mag = R.conv_terms(dy, b["wd"], None, b["res"], transposed=True)
        R.exact("stage out", out_mag.max(), 1 / 256)
        R.exact("stage terms gz y", out_mag.max() * 3.0, 1 / 1024)                           # gz = out / 4, |y| <= 3
        R.exact("stage terms g min(z, 0)", out_mag.max() * zmax, 1 / 512)                    # z in halves


# ------------------------------------------------------------------------------------------------ pinned activation signs
@pytest.mark.parametrize("case", R.BLOCK_CASES)
def test_pinned_share_stays_within_its_cap(case):
    (B, H, W), _, _ = R.CASES[case]
    n = B * H * W
    p = R.block_params(11)
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(B, H, W, 64, generator=gen, dtype=D).float().double()
    y1 = R.conv(h, p["w1"], p["b1"])
    pin, count = R.pinned(y1, p["g1"], p["be1"], n)
    assert count <= R.PIN_CAP * y1.numel() and int((pin != 0).sum()) == count


def test_guarded64_sees_a_stray_write():
    g = R.Guarded64("cpu")
    a = g.empty(3, 64, 2)
    assert a.storage_offset() % 2 == 0 and float(a.abs().sum()) == 0.0
    g.check()
    g = R.Guarded64("cpu")
    a = g.put(torch.ones(5, 4))
    g.bufs[0][0][R.GUARD64 + 20] = 0.0
    with pytest.raises(AssertionError):
        g.check()
