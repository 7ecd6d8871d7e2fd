"""GPU: the band conv kernel's ACCUMULATOR mode (csrc/conv_band.hip conv_band_kernel, BandAcc in csrc/conv_epilogue.h; entries
sst_conv_fwd_acc / sst_conv_dgrad_fused_acc) held to plain torch fp64 on the CPU, launch by launch: the forward epilogue that adds
the BatchNorm sums into fp64 accumulators, the forward prologue that derives the affine of its input from them (affine_from_acc, in its
late and early placement) and publishes mean / rstd / scale / shift and the running statistics once, the backward prologue that derives
cA / cB / cC and publishes dgamma / dbeta / dslope, and the backward epilogue.  The references are tests/band_acc_refs.py (held to
F.batch_norm / F.conv2d / autograd by tests/test_band_acc_refs.py on the CPU).

Cases (band_acc_refs.CASES: (B, H, W) -> NB blocks, R rows, patch pixels; each test first establishes the route: sst_conv_acc_supported,
sst_conv_stat_tiles == B H / R, and sst_debug_band_launches rises by one per call):
  a (5, 6, 24)   3, 2, 104   one load batch: the plain instance reduces the accumulators BEHIND the patch loads (nit <= UN)
  b (3, 2, 48)   3, 1, 150   nit = 10 > UN: reduction first; a top and a bottom image border in every band
  c (2, 8, 12)   3, 4, 84    four-row bands              d (2, 6, 8)   3, 6, 80   W = 8, a 16-pixel block spans two rows
  e (2, 4, 36)   9, 4, 228   NB = 9 by fall-through      f (1, 16, 9)  9, 16, 198 odd W, B = 1: only replica 0 is written
  g (2, 6, 24) with SST_CONV_BAND=9: 9, 6, 208           h (17, 2, 48) 3, 1, 150  B > 16: replica 0 receives two images
Cout = 64 and nrep = 16 everywhere; a and e also at Cout = 32 (two channel groups) and 16 (the publisher is the only group), a and h
also at nrep 1, 4, 5 (the `part + 4k < nrep` guards).  nrep is ops.ACC_NREP, set per test.

Rules:
  integer data        x, w, bias, g, saved y small integers, slope 0.25, scales in {0.5, 1, 2}, integer shifts; hand-written
                      accumulators that make every derived coefficient a small dyadic number (rstd exactly 0.5 / 1 / 2: IEEE sqrt and
                      division).  test_band_acc_refs.py asserts that every fp32 partial sum stays below 2^24 in its unit, so y, g, h,
                      dy, mean, rstd, scale, shift, dgamma, dbeta, dslope and every word of st_acc / bw_st_acc, PER REPLICA, equal fp64
                      bit for bit; replicas >= B and word 3 of the backward rows stay 0.0.
  random data, convs  norm-wise rel_err < 2e-5 (test_kernels_gpu.TOL) and elementwise |hip - fp64| <= k 2^-24 terms, k = 9 * 64 + 8 = 584
                      (576 FMAs, the other 8: affine, slope, bias, residual, the K-partial adds).  The truth is the fp64 conv of the
                      input transformed with the PUBLISHED fp32 scale / shift read back (backward: of the stored dy read back), so the
                      conv is held apart from the statistics.
  side outputs        h = fma(1, x, fma(kB, y2, kC)): k = 2, terms |x| + |y2 kB| + |kC|.  dy = fma(cA, gz, fma(cB, y, cC)) with
                      coefficients formed in fp32 from the fp64 sums (the kernel does not publish them): k = 10 (gz = g slope 1, the
                      two FMAs 2, cA 1, cB 3, cC 3 over its two products), terms |cA gz| + |cB y| + |cA m1| + |cA rstd mean m2|.
  accumulators        per replica against fp64 sums over the kernel's own stored fp32 output: sum of squares and the three backward
                      sums within k = 2 roundings of sum |term| (terms formed in fp32: the product, the slope multiply; summed in fp64),
                      the plain sum within k = R W roundings of sum |y| (the band total is an fp32 sum of R W values).
  published           mean, rstd, scale, shift, run_mean, run_var, dgamma, dbeta, dslope: conftest.assert_fp64_truth against the
                      restatement in fp32 / fp64 on the accumulators the launch read; mean within 1e-4, rstd within 2e-5 norm-wise.
                      run_var = (1 - m) rv + m (float)(M2 / (n - 1)): 6 roundings (m, 1 - m, the cast, two products, the add), all
                      terms positive -> rtol = 6 * 2^-24, atol = 0, against the restatement on the accumulators read AND against
                      F.batch_norm in fp64 on the rows they are the sums of (hand-written: the virtual rows; chained launches: the
                      stored y, rtol 8 * 2^-24: 2 more for the fp32 band totals of the producer, whose effect on run_var is
                      m * 2 mean^2 / var * |dA / A| ~ 0.1 * 2 * 0.3 * 2 * 2^-24 at this data).  n - 1 against n moves run_var by
                      m / n >= 6e-5 (test_band_acc_refs).  Two updates instead of one must FAIL the same comparison.
  large mean          the data of test_kernels_gpu.test_bn_stats_large_mean through producer and consumer: rstd within 1e-4.

Worst figures seen on the MI355X over all cases (run with -s for the running table):
  convs: elementwise |hip - fp64| / (2^-24 terms) 2.30 (bound 584), norm-wise 2.2e-7;  h 1.85 (bound 2);  dy 2.71 (bound 10), norm-wise 3.9e-8
  accumulators, as a share of their bound: plain sum 0.037 (k = R W), sum of squares 6e-9 (k = 2: the squares are exact in fp64),
    sum gz 0.034, sum gz y 0.21, sum g min(z, 0) 0.92 (k = 2 each; the last sum has one or two terms in channels whose z is rarely negative)
  published: mean 3.0e-8, rstd 4.7e-8 norm-wise;  run_var 2.12 * 2^-24 against the restatement and against F.batch_norm (bounds 6 and 8)
  residual block against fp64 autograd: worst 1.3e-6 (dslope; the fp32 autograd itself 1.5e-6)
  large mean: rstd error 6.4e-5 in accumulator mode, 6.4e-5 in tile mode (bound 1e-4)
Arithmetic-only mutants of the library (scratch builds, not kept): n for n - 1 in run_var fails test_consumer (36),
test_producer_consumer_chain (18) and test_residual_block_end_to_end (3); without the affine_from_acc() call of the nit > UN path
test_consumer (10), the chain (5) and the block (1) fail at cases b and h; the flipped sign in cC fails test_backward_stage (36) and the
block (3).
"""
import pytest
import torch
import torch.nn.functional as F

import band_acc_refs as R
import glue_refs as G
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
D, F32 = torch.float64, torch.float32
U24 = G.U24
K_RUNVAR_CHAIN = 8
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


def lib():
    from srganst import _abi
    return _abi.lib()


def dev(t):
    return None if t is None else t.detach().to(F32).contiguous().cuda()


def c64(t):
    return t.detach().cpu().double()


def worst(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def show(title):
    print(f"\n[{title}] " + "  ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


class Route:
    """Establishes the route of a config and counts band launches."""

    def __init__(self, ops, monkeypatch, config):
        case, cout, nrep = config
        (B, H, W), want, (nb, rr, patch) = R.CASES[case]
        if want:
            monkeypatch.setenv("SST_CONV_BAND", want)
        self.L = lib()
        assert self.L.sst_conv_acc_supported(B, H, W, 64, cout, 3, 1) == 1
        assert self.L.sst_conv_stat_tiles(B, H, W, 64, cout, 3, 1) == B * H // rr
        monkeypatch.setattr(ops, "ACC_NREP", nrep)
        self.n0 = self.L.sst_debug_band_launches()

    def launched(self, k):
        assert self.L.sst_debug_band_launches() == self.n0 + k, "one band-kernel launch per call"


# ================================================================================================ comparisons
def same(name, hip, ref64):
    hip = hip.detach().cpu()
    assert tuple(hip.shape) == tuple(ref64.shape), f"{name}: shape {tuple(hip.shape)} / {tuple(ref64.shape)}"
    if not torch.equal(hip.double(), ref64.double()):
        bad = (hip.double() != ref64.double()).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {ref64.numel()} elements differ from fp64, first at {bad[0].tolist()}: "
                             f"hip {hip[tuple(bad[0])].item()} ref {ref64[tuple(bad[0])].item()}")


def check_conv(name, hip, staged, w, bias, res, integer, transposed=False):
    """A conv output against the fp64 conv of what was staged."""
    ref = (R.dgrad if transposed else R.conv)(staged, w) + (0 if bias is None else bias) + (0 if res is None else res)
    if integer:
        return same(name, hip, ref)
    e = rel_err(hip.cpu(), ref)
    worst("conv norm-wise", e)
    assert e < TOL, f"{name}: |hip - fp64| / |fp64| = {e:.3e} >= {TOL}"
    worst("conv elementwise", G.assert_elementwise(name, hip, ref, R.conv_terms(staged, w, bias, res, transposed), R.K_CONV))


def check_rows(name, acc, ref, mag, ks, integer, B, words):
    """Accumulator rows [nrep, C, words] per replica: |acc - ref| <= ks[word] 2^-24 mag."""
    acc = c64(acc)
    nrep = acc.shape[0]
    if B < nrep:
        assert bool((acc[B:] == 0.0).all()), f"{name}: a replica >= B = {B} was written"
    if integer:
        return same(name, acc, ref)
    assert bool(torch.isfinite(acc).all()), f"{name}: non-finite accumulator"
    for wd, k in enumerate(ks):
        err, bound = (acc[..., wd] - ref[..., wd]).abs(), k * U24 * mag[..., wd]
        worst(f"{words[wd]} / bound", float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound + 1e-300).all()), f"{name} word {wd}: {int((err > bound).sum())} rows off by more than {k} roundings of sum |term|"


def check_fwd_acc(name, st, y_hip, nrep, rw, integer, y_ref=None):
    ref, mag = R.fwd_acc_of(y_ref if integer else c64(y_hip), nrep)
    check_rows(name, st, ref, mag, (rw, R.K_SUMSQ), integer, y_hip.shape[0], ("sum", "sum sq"))


def check_bwd_acc(name, st, out_hip, ysave, esc, esh, slope, act, nrep, integer, out_ref=None):
    ref, mag = R.bwd_acc_of(out_ref if integer else c64(out_hip), ysave, esc, esh, slope, act, nrep)
    assert bool((c64(st)[..., 3] == 0.0).all()), f"{name}: word 3 was written"
    check_rows(name, st, ref, mag, (2, 2, 2), integer, out_hip.shape[0], ("sum gz", "sum gz y", "sum g min(z,0)"))


def within(hip, ref, k):
    return bool(((c64(hip) - ref).abs() <= k * U24 * ref.abs()).all())


def check_published(name, pub, run, acc64, n, gamma, beta, rm0, rv0, exact=None, rows=None, k_rows=R.K_RUNVAR):
    """mean / rstd / scale / shift (pub) and the running buffers (run) of ONE consumer launch that read the accumulators acc64.
    rows [n, C]: the values the accumulators are the sums of."""
    t64, t32 = (R.fwd_finalize(acc64, n, gamma, beta, rm0, rv0, dt) for dt in (D, F32))
    if pub is not None:
        for k, hip in zip(("mean", "rstd", "scale", "shift"), pub):
            if exact is not None:
                same(f"{name} {k}", hip, exact[k])
            else:
                assert_fp64_truth(f"{name} {k}", hip.cpu(), t32[k], t64[k])
        if exact is None:
            e_m, e_r = rel_err(pub[0].cpu(), t64["mean"]), rel_err(pub[1].cpu(), t64["rstd"])
            worst("mean", e_m), worst("rstd", e_r)
            assert e_m < 1e-4 and e_r < 2e-5, f"{name}: mean {e_m:.3e} (1e-4) rstd {e_r:.3e} (2e-5)"
    if run is not None:
        for k, hip in zip(("run_mean", "run_var"), run):
            assert_fp64_truth(f"{name} {k}", hip.cpu(), t32[k], t64[k])
        worst("run_var / 2^-24", float(((c64(run[1]) - t64["run_var"]).abs() / (U24 * t64["run_var"].abs())).max()))
        assert within(run[1], t64["run_var"], R.K_RUNVAR), f"{name}: run_var off by more than {R.K_RUNVAR} roundings"
        e_rm = (c64(run[0]) - t64["run_mean"]).abs()                                   # signed terms: counted in their magnitudes
        assert bool((e_rm <= R.K_RUNVAR * U24 * ((1 - R.MOMENTUM) * rm0.abs() + R.MOMENTUM * t64["mean"].abs())).all()), f"{name}: run_mean"
        twice = R.fwd_finalize(acc64, n, gamma, beta, t64["run_mean"], t64["run_var"], D)
        assert not within(run[1], twice["run_var"], R.K_RUNVAR), f"{name}: the running statistics moved twice"
        if rows is not None:
            rm, rv = rm0.clone(), rv0.clone()
            F.batch_norm(rows, rm, rv, None, None, True, R.MOMENTUM, R.EPS)
            worst("run_var vs F.batch_norm / 2^-24", float(((c64(run[1]) - rv).abs() / (U24 * rv.abs())).max()))
            assert within(run[1], rv, k_rows), f"{name}: run_var is not F.batch_norm's within {k_rows} roundings (n - 1 or n?)"


def check_stage(name, dy, pubs, g, y, isc, ish, slope, act, acc64, mean, rstd, gamma, n, integer, report):
    """A backward stage's prologue: the published dgamma / dbeta / dslope (pubs: name -> tensor) and the side output dy against the
    restatement on the accumulators the launch read.  -> the fp64 dy."""
    t64, t32 = (R.bwd_finalize(acc64[..., :3], n, mean, rstd, gamma, dt) for dt in (D, F32))
    dy_ref = R.staged_bwd(g, y, isc, ish, slope, act, t64)
    if integer:
        for k, hip in pubs.items():
            same(f"{name} {k}", hip, t64[k])
        same(f"{name} dy", dy, dy_ref)
        return dy_ref
    for k, hip in pubs.items():
        assert_fp64_truth(f"{name} {k}", hip.cpu(), t32[k], t64[k], report)
    gz = R.staged_bwd(g, y, isc, ish, slope, act)
    S = R.totals(acc64)
    m1, m2 = S[:, 0] / n, rstd * (S[:, 1] - mean * S[:, 0]) / n
    terms = (t64["cA"] * gz).abs() + (t64["cB"] * y).abs() + (t64["cA"] * m1).abs() + (t64["cA"] * rstd * mean * m2).abs()
    worst("dy elementwise", G.assert_elementwise(f"{name} dy", dy, dy_ref, terms, R.K_DY_ACC))
    e = rel_err(dy.cpu(), dy_ref)
    worst("dy norm-wise", e)
    assert e < TOL, f"{name} dy: {e:.3e}"
    return dy_ref


def pub_bufs(gd):
    return tuple(gd.empty(64) for _ in range(4))          # sentinel-filled: an unpublished value fails its comparison


# ================================================================================================ form 1: producer only
@pytest.mark.parametrize("integer", [True, False], ids=["int", "rnd"])
@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_producer(ops, monkeypatch, config, integer):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    d = R.fwd_data(config, integer)
    wp = ops.pack_conv(dev(d["w"]), 0)
    slope_d = dev(torch.tensor([d["slope"]]))
    for act in (0, 1):
        gd, g64 = G.Guarded(), R.Guarded64()
        st = g64.empty(nrep, cout, 2)
        with gd.patch(ops):
            y, h = ops.conv_fwd_acc(dev(d["x"]), wp, cout, bias=dev(d["bias"]), in_slope=slope_d if act else None, in_act=act, st_acc=st)
        g64.check()
        rt.launched(act + 1)
        assert h is None
        staged = R.staged_fwd(d["x"], None, None, d["slope"], act)
        check_conv(f"y act={act}", y, staged, d["w"], d["bias"], None, integer)
        check_fwd_acc(f"st_acc act={act}", st, y, nrep, rr * W, integer, R.conv(staged, d["w"], d["bias"]))
    show("producer")


# ================================================================================================ form 2: consumer on hand-written accumulators
@pytest.mark.parametrize("integer", [True, False], ids=["int", "rnd"])
@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_consumer(ops, monkeypatch, config, integer):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    d = R.fwd_data(config, integer)
    hw = R.hand_fwd_acc(nrep, n, 42, integer)
    wp = ops.pack_conv(dev(d["w"]), 0)
    slope_d = dev(torch.tensor([d["slope"]]))
    gamma_d, beta_d = dev(hw["gamma"]), dev(hw["beta"])
    launches = 0
    for form, in2, act in (("prelu", None, 1), ("none", None, 0), ("residual", d["x2"], 0)):
        first = None
        for with_pub, with_run in ((True, True), (False, True), (True, False), (False, False)):
            gd, g64 = G.Guarded(), R.Guarded64()
            in_acc, st = g64.put(hw["acc"]), g64.empty(nrep, cout, 2)
            pub = pub_bufs(gd) if with_pub else None
            run = (gd.put(d["rm"]), gd.put(d["rv"])) if with_run else None
            with gd.patch(ops):
                y, h = ops.conv_fwd_acc(dev(d["x"]), wp, cout, in2=dev(in2), bias=dev(d["bias"]), in_slope=slope_d if act else None, in_act=act,
                                        in_acc=in_acc, in_bn=(gamma_d, beta_d), n=float(n), out_stats=pub, run_stats=run, st_acc=st)
            g64.check()
            launches += 1
            rt.launched(launches)
            name = f"{form} pub={with_pub} run={with_run}"
            assert torch.equal(in_acc.cpu(), hw["acc"]), f"{name}: the consumer wrote its input accumulators"
            check_published(name, pub, run, hw["acc"], n, hw["gamma"], hw["beta"], d["rm"], d["rv"],
                            exact=R.exact_affine(hw) if integer else None, rows=hw.get("yv"))
            if first is None:
                sc, sh = c64(pub[2]), c64(pub[3])
                if in2 is None:
                    staged = R.staged_fwd(d["x"], sc, sh, d["slope"], act)
                    if act and not integer:
                        z64 = d["x"] * sc + sh
                        _, cnt = G.undecided_signs(d["x"].reshape(n, 64), sc, sh, z64.reshape(n, 64))
                        assert cnt <= R.PIN_CAP * z64.numel()
                    assert h is None
                else:
                    staged = R.staged_res(d["x"], in2, sc, sh)
                    if integer:
                        same(f"{name} h", h, staged)
                    else:
                        worst("h elementwise", G.assert_elementwise(f"{name} h", h, staged, d["x"].abs() + (in2 * sc).abs() + sh.abs(), R.K_H))
                check_conv(f"{name} y", y, staged, d["w"], d["bias"], None, integer)
                first = (y, h, run)
                y_ref = R.conv(staged, d["w"], d["bias"])
            else:
                assert torch.equal(y, first[0]), f"{name}: y depends on which side outputs are asked for"
                assert h is None or torch.equal(h, first[1])
                if run is not None:
                    assert torch.equal(run[0], first[2][0]) and torch.equal(run[1], first[2][1])
            check_fwd_acc(f"{name} st_acc", st, y, nrep, rr * W, integer, y_ref)
    show("consumer")


# ================================================================================================ forms 3 and 6: the chained launches
def block_forward(ops, rt, p, h, cout, nrep, rr):
    """conv_a -> (BN1 + PReLU on load) conv_b -> (h + BN2(y2) on load) conv_c exactly as gen_graph.forward chains them; no host touch of
    the accumulators in between.  Checks every launch against fp64 and returns what the backward needs."""
    B, H, W, _ = h.shape
    n, rw = B * H * W, rr * W
    gd, g64 = G.Guarded(), R.Guarded64()
    acc1, acc2, acc3 = g64.empty(nrep, 64, 2), g64.empty(nrep, 64, 2), g64.empty(nrep, cout, 2)
    pub1, pub2 = pub_bufs(gd), pub_bufs(gd)
    run1, run2 = (gd.put(p["rm1"]), gd.put(p["rv1"])), (gd.put(p["rm2"]), gd.put(p["rv2"]))
    wp = [ops.pack_conv(dev(p[k]), 0) for k in ("w1", "w2", "w3")]
    slope_d, h_d = dev(p["slope"]), dev(h)
    bn = lambda k: (dev(p["g" + k]), dev(p["be" + k]))
    with gd.patch(ops):
        y1, _ = ops.conv_fwd_acc(h_d, wp[0], 64, bias=dev(p["b1"]), st_acc=acc1)
        y2, _ = ops.conv_fwd_acc(y1, wp[1], 64, in_slope=slope_d, in_act=1, in_acc=acc1, in_bn=bn("1"), n=float(n), out_stats=pub1,
                                 run_stats=run1, st_acc=acc2)
        y3, hp = ops.conv_fwd_acc(h_d, wp[2], cout, in2=y2, in_acc=acc2, in_bn=bn("2"), n=float(n), out_stats=pub2, run_stats=run2,
                                  st_acc=acc3)
    g64.check()
    rt.launched(3)
    slope = float(p["slope"])
    check_conv("y1", y1, h, p["w1"], p["b1"], None, False)
    check_fwd_acc("acc1", acc1, y1, nrep, rw, False)
    check_published("BN1", pub1, run1, c64(acc1), n, p["g1"], p["be1"], p["rm1"], p["rv1"], rows=c64(y1).reshape(n, 64), k_rows=K_RUNVAR_CHAIN)
    m, v = G.batch_stats(c64(y1).reshape(n, 64))
    assert rel_err(pub1[0].cpu(), m) < 1e-4 and rel_err(pub1[1].cpu(), 1 / torch.sqrt(v + R.EPS)) < 2e-5
    check_conv("y2", y2, R.staged_fwd(c64(y1), c64(pub1[2]), c64(pub1[3]), slope, True), p["w2"], None, None, False)
    check_fwd_acc("acc2", acc2, y2, nrep, rw, False)
    check_published("BN2", pub2, run2, c64(acc2), n, p["g2"], p["be2"], p["rm2"], p["rv2"], rows=c64(y2).reshape(n, 64), k_rows=K_RUNVAR_CHAIN)
    m, v = G.batch_stats(c64(y2).reshape(n, 64))
    assert rel_err(pub2[0].cpu(), m) < 1e-4 and rel_err(pub2[1].cpu(), 1 / torch.sqrt(v + R.EPS)) < 2e-5
    sc2, sh2 = c64(pub2[2]), c64(pub2[3])
    staged = R.staged_res(h, c64(y2), sc2, sh2)
    worst("h elementwise", G.assert_elementwise("hp", hp, staged, h.abs() + (c64(y2) * sc2).abs() + sh2.abs(), R.K_H))
    check_conv("y3", y3, staged, p["w3"], None, None, False)
    check_fwd_acc("acc3", acc3, y3, nrep, rw, False)
    return dict(y1=y1, y2=y2, y3=y3, hp=hp, pub1=pub1, pub2=pub2, run1=run1, run2=run2, slope_d=slope_d, h_d=h_d)


def block_inputs(config):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(B, H, W, 64, generator=gen, dtype=D).float().double()
    up = torch.randn(B, H, W, cout, generator=gen, dtype=D).float().double()
    return R.block_params(11, cout), h, up


@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_producer_consumer_chain(ops, monkeypatch, config):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    p, h, _ = block_inputs(config)
    block_forward(ops, rt, p, h, cout, nrep, rr)
    show("chain")


@pytest.mark.parametrize("case", R.BLOCK_CASES)
def test_residual_block_end_to_end(ops, monkeypatch, case):
    config = (case, 64, 16)
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    p, h, up = block_inputs(config)
    f = block_forward(ops, rt, p, h, cout, nrep, rr)
    gd, g64 = G.Guarded(), R.Guarded64()
    bacc1, bacc2 = g64.empty(nrep, 64, 4), g64.empty(nrep, 64, 4)
    dg1, db1, dsl, dg2, db2 = gd.empty(64), gd.empty(64), gd.empty(1), gd.empty(64), gd.empty(64)
    wd = {k: ops.pack_conv(dev(p[k]), 1) for k in ("w1", "w2", "w3")}
    (m1, r1, s1, t1), (m2, r2, _, _) = f["pub1"], f["pub2"]
    with gd.patch(ops):                                                     # gen_graph.backward: conv2's data-gradient, stage 2, stage 1
        dhp, _ = ops.conv_dgrad_fused_acc(dev(up), wd["w3"], 64, epi_y=f["y2"], bw_st_acc=bacc2)
        dp1, dy2 = ops.conv_dgrad_fused_acc(dhp, wd["w2"], 64, y2=f["y2"], epi_y=f["y1"], epi_scale=s1, epi_shift=t1, epi_slope=f["slope_d"],
                                            epi_act=1, bw_in_acc=bacc2, bn=(m2, r2, dev(p["g2"])), n=float(n), dgamma=dg2, dbeta=db2,
                                            bw_st_acc=bacc1)
        dh, dy1 = ops.conv_dgrad_fused_acc(dp1, wd["w1"], 64, y2=f["y1"], in_scale=s1, in_shift=t1, in_slope=f["slope_d"], in_act=1,
                                           residual=dhp, bw_in_acc=bacc1, bn=(m1, r1, dev(p["g1"])), n=float(n), dgamma=dg1, dbeta=db1,
                                           dslope=dsl)
    g64.check()
    rt.launched(6)
    slope = float(p["slope"])
    check_bwd_acc("bacc2", bacc2, dhp, c64(f["y2"]), None, None, 0.0, 0, nrep, False)
    check_bwd_acc("bacc1", bacc1, dp1, c64(f["y1"]), c64(s1), c64(t1), slope, 1, nrep, False)
    report = []
    check_conv("dhp", dhp, up, p["w3"], None, None, False, transposed=True)
    check_stage("stage 2", dy2, dict(dgamma=dg2, dbeta=db2), c64(dhp), c64(f["y2"]), None, None, 0.0, 0, c64(bacc2), c64(m2), c64(r2), p["g2"], n,
                False, report)
    check_conv("dp1", dp1, c64(dy2), p["w2"], None, None, False, transposed=True)
    check_stage("stage 1", dy1, dict(dgamma=dg1, dbeta=db1, dslope=dsl), c64(dp1), c64(f["y1"]), c64(s1), c64(t1), slope, 1, c64(bacc1), c64(m1),
                c64(r1), p["g1"], n, False, report)
    check_conv("dh", dh, c64(dy1), p["w1"], None, c64(dhp), False, transposed=True)
    pin, cnt = R.pinned(R.conv(h, p["w1"], p["b1"]), p["g1"], p["be1"], n)
    assert cnt <= R.PIN_CAP * pin.numel()
    a64, a32 = R.block(h, p, up, D, pin), R.block(h, p, up, F32, pin)
    hip = dict(y1=f["y1"], y2=f["y2"], hp=f["hp"], y3=f["y3"], dhp=dhp, dy2=dy2, dy1=dy1, dh=dh, dgamma1=dg1, dbeta1=db1, dslope=dsl,
               dgamma2=dg2, dbeta2=db2, rm1=f["run1"][0], rv1=f["run1"][1], rm2=f["run2"][0], rv2=f["run2"][1])
    for k, v in hip.items():
        assert_fp64_truth("block " + k, v.cpu().reshape(a64[k].shape), a32[k], a64[k], report)
    G.print_report(f"residual block {case}", report)
    show("block")


# ================================================================================================ form 4: backward producer
@pytest.mark.parametrize("integer", [True, False], ids=["int", "rnd"])
@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_backward_producer(ops, monkeypatch, config, integer):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    b = R.bwd_data(config, integer)
    wd = ops.pack_conv(dev(b["wd"]), 1)
    slope_d = dev(torch.tensor([b["slope"]]))
    launches = 0
    for act in (0, 1):
        for with_aff in (False, True):
            for with_res in (False, True):
                gd, g64 = G.Guarded(), R.Guarded64()
                st = g64.empty(nrep, cout, 4)
                esc, esh = (b["esc"], b["esh"]) if with_aff else (None, None)
                res = b["res"] if with_res else None
                with gd.patch(ops):
                    out, dy = ops.conv_dgrad_fused_acc(dev(b["g"]), wd, cout, residual=dev(res), epi_y=dev(b["ysave"]), epi_scale=dev(esc),
                                                       epi_shift=dev(esh), epi_slope=slope_d if act else None, epi_act=act, bw_st_acc=st)
                g64.check()
                launches += 1
                rt.launched(launches)
                assert dy is None
                name = f"act={act} affine={with_aff} residual={with_res}"
                check_conv(name + " out", out, b["g"], b["wd"], None, res, integer, transposed=True)
                check_bwd_acc(name + " bw_st_acc", st, out, b["ysave"], esc, esh, b["slope"], act, nrep, integer,
                              R.dgrad(b["g"], b["wd"]) + (0 if res is None else res))
    show("backward producer")


# ================================================================================================ form 5: backward stage
STAGES = [  # in_act, dslope given, residual, a next stage (epi_y + bw_st_acc: epi_act, epi affine) or None: the block's last stage
    (1, True, True, (1, True)),
    (1, False, False, None),
    (0, False, True, (0, False)),
    (0, True, True, None),
]


@pytest.mark.parametrize("integer", [True, False], ids=["int", "rnd"])
@pytest.mark.parametrize("config", R.CONFIGS, ids=R.CONFIG_ID)
def test_backward_stage(ops, monkeypatch, config, integer):
    B, H, W, cout, nrep, n, rr = R.dims(config)
    rt = Route(ops, monkeypatch, config)
    b = R.bwd_data(config, integer)
    wd = ops.pack_conv(dev(b["wd"]), 1)
    slope_d = dev(torch.tensor([b["slope"]]))
    report = []
    for i, (act, with_dslope, with_res, nxt) in enumerate(STAGES):
        hb = R.hand_bwd_acc(nrep, n, 43, integer, act)
        gd, g64 = G.Guarded(), R.Guarded64()
        bw_in = g64.put(hb["acc"])
        st = g64.empty(nrep, cout, 4) if nxt else None
        dgam, dbet, dsl = gd.empty(64), gd.empty(64), gd.empty(1) if with_dslope else None
        res = b["res"] if with_res else None
        e_act, e_aff = nxt if nxt else (0, False)
        esc, esh = (b["esc"], b["esh"]) if e_aff else (None, None)
        isc, ish = (b["isc"], b["ish"]) if act else (None, None)
        with gd.patch(ops):
            out, dy = ops.conv_dgrad_fused_acc(dev(b["g"]), wd, cout, y2=dev(b["y2"]), in_scale=dev(isc), in_shift=dev(ish),
                                               in_slope=slope_d if act else None, in_act=act, residual=dev(res),
                                               epi_y=dev(b["ysave"]) if nxt else None, epi_scale=dev(esc), epi_shift=dev(esh),
                                               epi_slope=slope_d if e_act else None, epi_act=e_act, bw_in_acc=bw_in,
                                               bn=(dev(hb["mean"]), dev(hb["rstd"]), dev(hb["gamma"])), n=float(n), dgamma=dgam, dbeta=dbet,
                                               dslope=dsl, bw_st_acc=st)
        g64.check()
        rt.launched(i + 1)
        name = f"stage {i}"
        assert torch.equal(bw_in.cpu(), hb["acc"]), f"{name}: the stage wrote its input accumulators"
        pubs = dict(dgamma=dgam, dbeta=dbet, **(dict(dslope=dsl) if with_dslope else {}))
        dy_ref = check_stage(name, dy, pubs, b["g"], b["y2"], isc, ish, b["slope"], act, hb["acc"], hb["mean"], hb["rstd"], hb["gamma"], n,
                             integer, report)
        check_conv(f"{name} out", out, dy_ref if integer else c64(dy), b["wd"], None, res, integer, transposed=True)
        if nxt:
            check_bwd_acc(f"{name} bw_st_acc", st, out, b["ysave"], esc, esh, b["slope"], e_act, nrep, integer,
                          R.dgrad(dy_ref, b["wd"]) + (0 if res is None else res))
    G.print_report("backward stage", report)
    show("backward stage")


# ================================================================================================ large mean
def test_large_mean_through_the_accumulators(ops, monkeypatch):
    """The data of test_kernels_gpu.test_bn_stats_large_mean ((4, 24, 24), identity weights, bias 100: |mean| = 100 std) through an
    accumulator-mode producer and consumer: the published rstd within the 1e-4 that tile mode is held to.  Prints both modes' errors."""
    B, H, W, C = 4, 24, 24, 64
    assert R.band_rows(H, W) == (3, 2, 104) and lib().sst_conv_acc_supported(B, H, W, C, C, 3, 1) == 1
    monkeypatch.setattr(ops, "ACC_NREP", 16)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c, 1, 1] = 1.0
    bias = torch.full((C,), 100.0)
    xd, wp = x.permute(0, 2, 3, 1).contiguous().cuda(), ops.pack_conv(w.cuda())
    truth = 1 / torch.sqrt((x + 100.0).double().var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    gd, g64 = G.Guarded(), R.Guarded64()
    st, pub = g64.empty(16, C, 2), pub_bufs(gd)
    n0 = lib().sst_debug_band_launches()
    with gd.patch(ops):
        y, _ = ops.conv_fwd_acc(xd, wp, C, bias=bias.cuda(), st_acc=st)
        ops.conv_fwd_acc(y, wp, C, in_acc=st, in_bn=(torch.ones(C).cuda(), torch.zeros(C).cuda()), n=float(B * H * W), out_stats=pub)
    g64.check()
    assert lib().sst_debug_band_launches() == n0 + 2
    _, _, stats, cnt = ops.conv_fwd(xd, wp, C, 3, 1, bias=bias.cuda(), want_stats=True)            # tile mode, as test_bn_stats_large_mean
    _, rstd_tile, _, _ = ops.bn_finalize(stats, cnt, torch.ones(C).cuda(), torch.zeros(C).cuda())
    e_acc, e_tile = rel_err(pub[1].cpu(), truth), rel_err(rstd_tile.cpu(), truth)
    print(f"\n[large mean] rstd error: accumulator mode {e_acc:.3e}, tile mode {e_tile:.3e} (bound 1e-4)")
    assert e_acc < 1e-4, f"accumulator mode: {e_acc:.3e} (tile mode {e_tile:.3e})"


# ================================================================================================ refused calls
def test_refused_calls_launch_nothing(ops, monkeypatch):
    from srganst._abi import HipPathError
    L = lib()
    monkeypatch.setattr(ops, "ACC_NREP", 16)
    n0 = L.sst_debug_band_launches()
    w = torch.zeros(64, 64, 3, 3).cuda()
    wp, wd = ops.pack_conv(w, 0), ops.pack_conv(w, 1)
    acc2, acc4 = torch.zeros(16, 64, 2, dtype=D).cuda(), torch.zeros(16, 64, 4, dtype=D).cuda()
    v64 = torch.ones(64).cuda()

    def refused(call, *a, **kw):
        with pytest.raises(HipPathError):
            call(*a, **kw)
        torch.cuda.synchronize()
        assert L.sst_debug_band_launches() == n0
        assert float(acc2.abs().sum()) == 0.0 and float(acc4.abs().sum()) == 0.0

    for B, H, W in R.REFUSED_SHAPES:
        assert L.sst_conv_acc_supported(B, H, W, 64, 64, 3, 1) == 0
        x = torch.zeros(B, H, W, 64).cuda()
        refused(ops.conv_fwd_acc, x, wp, 64, st_acc=acc2)
        refused(ops.conv_dgrad_fused_acc, x, wd, 64, epi_y=x, bw_st_acc=acc4)
    x = torch.zeros(2, 6, 24, 64).cuda()
    assert L.sst_conv_acc_supported(2, 6, 24, 128, 64, 3, 1) == 0                                   # Cin = 128
    x128 = torch.zeros(2, 6, 24, 128).cuda()
    wp128 = ops.pack_conv(torch.zeros(64, 128, 3, 3).cuda(), 0)
    refused(ops.conv_fwd_acc, x128, wp128, 64, st_acc=acc2)
    refused(ops.conv_dgrad_fused_acc, x128, wp128, 64, epi_y=x, bw_st_acc=acc4)
    for nrep in (0, 17):
        monkeypatch.setattr(ops, "ACC_NREP", nrep)
        refused(ops.conv_fwd_acc, x, wp, 64, st_acc=acc2)
        refused(ops.conv_dgrad_fused_acc, x, wd, 64, epi_y=x, bw_st_acc=acc4)
    monkeypatch.setattr(ops, "ACC_NREP", 16)
    refused(ops.conv_fwd_acc, x, wp, 64)                                                            # no accumulator at all
    refused(ops.conv_fwd_acc, x, wp, 64, in_acc=acc2, n=288.0, st_acc=acc2)                         # in_acc without gamma / beta
    refused(ops.conv_fwd_acc, x, wp, 64, in_acc=acc2, in_bn=(v64, v64), n=0.0)                      # ... without n
    refused(ops.conv_dgrad_fused_acc, x, wd, 64, bw_st_acc=acc4)                                    # bw_st_acc without epi_y
    refused(ops.conv_dgrad_fused_acc, x, wd, 64, y2=x, bw_in_acc=acc4, n=288.0, dgamma=v64, dbeta=v64)      # bw_in_acc without mean / rstd / gamma

    class NoSideOutput:                                                                             # y2 without dy_out: the wrapper always
        def empty_like(self, t, **kw):                                                              # allocates dy, so take that away
            return None

        def __getattr__(self, name):
            return getattr(torch, name)
    monkeypatch.setattr(ops, "torch", NoSideOutput())
    refused(ops.conv_dgrad_fused_acc, x, wd, 64, y2=x, epi_y=x, bw_st_acc=acc4)
