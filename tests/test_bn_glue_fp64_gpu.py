"""GPU: the BatchNorm / activation glue kernels (csrc/bn_elem.hip) held to plain torch fp64 on the CPU, at the shapes where their
loops, tails and branches change: the backward chain reduce -> finalize -> apply, both finalize kernels on the same partials, the
grouped forms, bwd_apply's coefficient reload and unrolled batch, the forward finalizes, and the elementwise helpers.

Rules (tests/glue_refs.py holds the formulas, tests/test_glue_references.py holds those to autograd on the CPU):
  data movement / selection            bitwise
  elementwise fp32 chains              |hip - ref64| <= k * 2^-24 * sum|terms| per element, k = fp32 roundings, written at each use
  reductions and gradients through     conftest.assert_fp64_truth: rel err <= max(1e-3, 3 x rel err of the same formula in fp32 torch)
Every output lives between two sentinel-filled guard bands that are checked after the launches.  Run with -s for the error tables."""
import itertools

import pytest
import torch

import glue_refs as G
from conftest import assert_fp64_truth, rel_err, truth_bound  # noqa: F401  (rel_err / truth_bound: printed by the tables)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


def dev(t):
    return None if t is None else t.detach().to(torch.float32).contiguous().cuda()


CONDS = ("normal", "mean1e3", "const")


def make_rows(seed, R, C, cond, k=0):
    """y [R, C] fp32 (held as fp64 values).  normal: mean O(1); mean1e3: |mean| / sigma = 1e3 per channel (the S1 - mean*S0
    cancellation the fp64 finalize exists for); const: channel C/2 constant (var = 0, rstd = 1/sqrt(eps)).  k: pass index of the
    grouped forms (mean k, scale 2^k on top)."""
    gen = torch.Generator().manual_seed(seed)
    sig = (torch.rand(C, generator=gen) + 0.5) * 2.0 ** k
    y = torch.randn(R, C, generator=gen) * sig + k
    if cond == "mean1e3":
        if R > 1:                                                # the ratio is the batch's own: standardise the draw per channel
            y = (y - y.mean(0)) / y.std(0, unbiased=False) * sig
        y = y + 1000.0 * sig * torch.where(torch.rand(C, generator=gen) > 0.5, 1.0, -1.0)
    else:
        y = y + 0.5 * torch.randn(C, generator=gen)
    if cond == "const":
        y[:, C // 2] = 0.75
    return y.float().double()


def affine_of(y, gamma, beta):
    """fp32 (mean, rstd, scale, shift) of the batch, rounded once from fp64 - what a correct forward finalize hands the backward."""
    mean, var = G.batch_stats(y)
    rstd = 1 / torch.sqrt(var + G.EPS)
    return mean.float(), rstd.float(), (gamma * rstd).float(), (beta - mean * gamma * rstd).float()


def params(seed, C):
    gen = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(C, generator=gen) + 0.5).float().double()
    beta = (0.3 * torch.randn(C, generator=gen)).float().double()
    return gamma, beta


# ================================================================================================ backward chain
CHAIN_C = [4, 8, 16, 64, 128, 256, 512, 1024]
CHAIN_R = [1, 3, 63, 288, 2305, 16 * 24 * 24]
CHAIN = list(itertools.product(CHAIN_C, CHAIN_R)) + [(64, 16 * 96 * 96)]
FLAGS = list(itertools.product((0, 1), repeat=3))                 # (g2 given, slope as a device scalar, accumulate)


@pytest.mark.parametrize("C, R", CHAIN)
def test_backward_chain_vs_fp64(ops, C, R):
    """bwd_reduce -> bwd_finalize -> bwd_apply against fp64 autograd of F.batch_norm(train) + F.prelu / F.leaky_relu, on the three
    data conditionings.  The flags (g2, device / constant slope, accumulate, act) rotate with the case index and the conditioning
    so that every flag value meets every C and every R across the grid; C > 64 with a device slope takes the wide finalize, a
    constant slope or act = 0 the 16-channel finalize, C <= 64 with a device slope the single-workgroup one.
    R = 1: the truth of dy and dgamma is exactly 0 (one value per channel), a relative error does not exist there: those two are
    held to the elementwise rule with k = 8 (g + g2, * slope, a = gamma*rstd, a*m1, the sum of cC, two fmaf of the apply, the
    accumulate) on sum|terms| = |cA gz| + |cB y| + |cC| resp. rstd (|S1| + |mean S0|) + |prefill|.  One row has no sigma either, so
    |mean| / sigma = 1e3 is not defined there: that conditioning runs as a second normal draw at R = 1.
    Where the sign of z is not decided by fp32 scale / shift (glue_refs.undecided_signs: a handful of elements at |mean| / sigma =
    1e3, none otherwise) both references take the branch those coefficients give; everywhere else they are F.prelu / F.leaky_relu."""
    idx = CHAIN.index((C, R))
    report, pinned = [], 0
    for ci, cond in enumerate(CONDS):
        has_g2, slope_dev, acc = FLAGS[(3 * idx + ci) % 8]
        act = int((idx + ci) % 4 != 3)
        seed = 1000 * idx + ci
        y = make_rows(seed, R, C, cond if R > 1 or cond != "mean1e3" else "normal")
        gen = torch.Generator().manual_seed(seed + 7)
        up = torch.randn(R, C, generator=gen).double()
        up2 = torch.randn(R, C, generator=gen).double() if has_g2 else None
        gamma, beta = params(seed + 9, C)
        slope_c = 0.2
        slope_t = torch.tensor([0.25], dtype=torch.float64) if slope_dev else None
        slope = slope_t if slope_dev else slope_c
        pre = {k: torch.randn(n, generator=gen).float().double() for k, n in (("dgamma", C), ("dbeta", C), ("dslope", 1))}
        want_slope = bool(act and slope_dev)
        tag = f"C={C} R={R} {cond} g2={has_g2} slope={'dev' if slope_dev else 'const'} act={act} acc={acc}"

        upt = up if up2 is None else up + up2
        mean, rstd, scale, shift = affine_of(y, gamma, beta)
        pin, npin = G.undecided_signs(y, scale, shift, G.bn_act(y, gamma, beta, 0.0, 0))
        pinned += npin
        r64 = G.chain_grads(y, upt, gamma, beta, slope, act, torch.float64, pin=pin)
        r32 = G.chain_grads(y.float(), upt.float(), gamma, beta, slope, act, torch.float32, pin=pin)
        gd = G.Guarded()
        with gd.patch(ops):
            part = ops.bwd_reduce(dev(up), dev(y), g2=dev(up2), scale=dev(scale), shift=dev(shift), slope=dev(slope_t),
                                  slope_const=slope_c, act=act)
            assert part.shape[0] == G.reduce_blocks(R, C)
            dgamma, dbeta = (gd.put(pre[k]) if acc else gd.empty(C) for k in ("dgamma", "dbeta"))
            dslope = (gd.put(pre["dslope"]) if acc else gd.empty(1)) if want_slope else None
            cA, cB, cC = ops.bwd_finalize(part, R, dev(mean), dev(rstd), dev(gamma), dgamma, dbeta, dslope, accumulate=bool(acc))
            dy = ops.bwd_apply(dev(up), dev(y), g2=dev(up2), scale=dev(scale), shift=dev(shift), slope=dev(slope_t),
                               slope_const=slope_c, act=act, cA=cA, cB=cB, cC=cC)
        got = {"dy": dy.cpu(), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}
        if want_slope:
            got["dslope"] = dslope.cpu()
        for k, h in got.items():
            add64 = pre[k] if (acc and k != "dy") else 0.0
            if R == 1 and k in ("dy", "dgamma"):
                assert float(r64[k].abs().max()) < 1e-12
                S = G.bwd_sums(upt, y, scale.double(), shift.double(), slope if act else 0.0, act)
                co = G.bwd_coeffs(S, mean.double(), rstd.double(), gamma, R)
                if k == "dy":
                    gz = G.bwd_gz(upt, y, scale.double(), shift.double(), slope if act else 0.0, act)[0]
                    terms = (co["cA"] * gz).abs() + (co["cB"] * y).abs() + co["cC"].abs()
                else:
                    terms = rstd.double() * (S[1].abs() + (mean.double() * S[0]).abs()) + (pre[k].abs() if acc else 0.0)
                G.assert_elementwise(f"{k} {tag}", h, r64[k] + add64, terms, 8)
            else:
                add32 = add64.float() if torch.is_tensor(add64) else 0.0
                assert_fp64_truth(f"{k} {tag}", h, (r32[k] + add32).double(), r64[k] + add64, report)
    G.print_report(f"backward chain C={C} R={R} ({pinned} of {3 * R * C} activation signs undecided in fp32)", report)


# ================================================================================================ the two slope finalizes
def _finalize_direct(ops, wide, part, n, mean, rstd, gamma, out, acc, scratch=None, counter=None):
    from srganst import _abi
    from srganst._abi import check, ptr, stream_ptr
    nblk, _, C = part.shape
    head = (ptr(part), nblk, C, float(n), ptr(mean), ptr(rstd), ptr(gamma), ptr(out["dgamma"]), ptr(out["dbeta"]), ptr(out["cA"]),
            ptr(out["cB"]), ptr(out["cC"]), ptr(out["dslope"]), int(acc))
    if wide:
        check(_abi.lib().sst_bwd_finalize_wide(*head, ptr(scratch), ptr(counter), stream_ptr()), "sst_bwd_finalize_wide")
    else:
        check(_abi.lib().sst_bwd_finalize(*head, stream_ptr()), "sst_bwd_finalize")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("C, R", [(128, 2305), (256, 288), (512, 63), (1024, 2305), (256, 16 * 24 * 24)])
def test_finalize_wide_against_single_workgroup(ops, C, R, acc):
    """sst_bwd_finalize_wide (one workgroup per 64 channels, last arriver sums the slope gradient) and sst_bwd_finalize (one
    workgroup) on the same partials: cA / cB / cC / dgamma / dbeta bit-equal, dslope equal to within the reassociation of the sum
    (bound: (C/64 + 16) roundings of sum_c |S2_c|: C/64 channel terms per thread, then the 16 + 4 steps of block_sum resp. the
    C/64 workgroup terms) and both within the fp64 rule; the counter word reads 0 afterwards; a second launch is bit-identical."""
    report = []
    y = make_rows(C + R, R, C, "mean1e3")
    gen = torch.Generator().manual_seed(C + R + 1)
    up = torch.randn(R, C, generator=gen).double()
    gamma, beta = params(C + R + 2, C)
    slope = torch.tensor([0.25], dtype=torch.float64)
    mean, rstd, scale, shift = affine_of(y, gamma, beta)
    pre = {k: torch.randn(n, generator=gen).float().double() for k, n in (("dgamma", C), ("dbeta", C), ("dslope", 1))}
    pin, _ = G.undecided_signs(y, scale, shift, G.bn_act(y, gamma, beta, 0.0, 0))
    r64 = G.chain_grads(y, up, gamma, beta, slope, 1, torch.float64, pin=pin)
    r32 = G.chain_grads(y.float(), up.float(), gamma, beta, slope, 1, torch.float32, pin=pin)
    S64 = G.bwd_sums(up, y, scale.double(), shift.double(), slope, 1)
    gd = G.Guarded()
    with gd.patch(ops):
        part = ops.bwd_reduce(dev(up), dev(y), scale=dev(scale), shift=dev(shift), slope=dev(slope), act=1)
    runs = {}
    for name, wide in (("single", False), ("wide", True), ("wide again", True)):
        out = {k: (gd.put(pre[k]) if acc else gd.empty(pre[k].shape)) if k in pre else gd.empty(C)
               for k in ("dgamma", "dbeta", "dslope", "cA", "cB", "cC")}
        scratch = gd.empty((C + 63) // 64)
        counter = gd.empty(1, dtype=torch.int32, fill=0)
        _finalize_direct(ops, wide, part, R, dev(mean), dev(rstd), dev(gamma), out, acc, scratch, counter)
        gd.check()
        assert int(counter.item()) == 0, "the last-arriver counter must be left zero"
        runs[name] = {k: v.cpu() for k, v in out.items()}
    for k in ("cA", "cB", "cC", "dgamma", "dbeta"):
        assert torch.equal(runs["single"][k], runs["wide"][k]), f"{k}: wide and single-workgroup finalize differ"
    for k in runs["wide"]:
        assert torch.equal(runs["wide"][k], runs["wide again"][k]), f"{k}: second launch differs"
    ds, dw = runs["single"]["dslope"].double(), runs["wide"]["dslope"].double()
    assert float((ds - dw).abs()) <= (C // 64 + 16) * G.U24 * float(S64[2].abs().sum() + (pre["dslope"].abs().sum() if acc else 0))
    for name in ("single", "wide"):
        for k in ("dgamma", "dbeta", "dslope"):
            add = pre[k] if acc else 0.0
            assert_fp64_truth(f"{k} {name} C={C} R={R} acc={acc}", runs[name][k], (r32[k] + (add.float() if acc else 0.0)).double(),
                              r64[k] + add, report)
    G.print_report(f"finalize wide / single C={C} R={R}", report)


# ================================================================================================ finalize on hand-made partials
@pytest.mark.parametrize("C", [5, 24, 64, 200])
@pytest.mark.parametrize("nblk", [1, 7, 63, 64, 100, 256])
def test_finalize_kernels_on_synthetic_partials(ops, C, nblk):
    """Both finalize kernels straight on random partials [nblk][3][C], at the edges of their thread layouts: fewer blocks than row
    lanes (64 for the 16-channel kernel, 16 for the other), block counts that are no multiple of them, channel counts that are no
    multiple of 16 / 64, BatchNorm mode and bias-only mode (mean = null) with accumulate.  Truth: the sums of the same partials and
    the coefficient formulas in fp64."""
    from srganst import _abi
    from srganst._abi import check, ptr, stream_ptr
    report = []
    gen = torch.Generator().manual_seed(100 * C + nblk)
    part = torch.randn(nblk, 3, C, generator=gen).float()
    part[:, 1] += 3.0 * part[:, 0]                               # S1 and mean*S0 of one size: the difference cancels
    mean = (3.0 + 0.1 * torch.randn(C, generator=gen)).float()
    rstd = (torch.rand(C, generator=gen) + 0.5).float()
    gamma = (torch.rand(C, generator=gen) + 0.5).float()
    pre = {k: torch.randn(n, generator=gen).float() for k, n in (("dgamma", C), ("dbeta", C), ("dslope", 1))}
    n = float(nblk * 37)

    def truth(dtype):
        S = part.to(dtype).sum(0)
        return G.bwd_coeffs(S, mean.to(dtype), rstd.to(dtype), gamma.to(dtype), n)
    r64, r32 = truth(torch.float64), truth(torch.float32)
    gd = G.Guarded()
    pd, md, rd, gad = dev(part), dev(mean), dev(rstd), dev(gamma)
    for kern, bn, acc in itertools.product(("f3", "f2", "wide"), (1, 0), (0, 1)):
        want_slope = kern != "f3"
        out = {k: (gd.put(pre[k]) if acc else gd.empty(pre[k].shape)) for k in ("dgamma", "dbeta", "dslope")}
        out.update({k: gd.empty(C) for k in ("cA", "cB", "cC")})
        scratch, counter = gd.empty((C + 63) // 64), gd.empty(1, dtype=torch.int32, fill=0)
        a = (ptr(pd), nblk, C, n, ptr(md) if bn else None, ptr(rd) if bn else None, ptr(gad) if bn else None,
             ptr(out["dgamma"]) if bn else None, ptr(out["dbeta"]), ptr(out["cA"]) if bn else None, ptr(out["cB"]) if bn else None,
             ptr(out["cC"]) if bn else None, ptr(out["dslope"]) if want_slope else None, acc)
        if kern == "wide":
            check(_abi.lib().sst_bwd_finalize_wide(*a, ptr(scratch), ptr(counter), stream_ptr()), "sst_bwd_finalize_wide")
        else:
            check(_abi.lib().sst_bwd_finalize(*a, stream_ptr()), "sst_bwd_finalize")
        untouched = {k: v.clone() for k, v in out.items()}
        gd.check()
        assert int(counter.item()) == 0
        tag = f"{kern} bn={bn} acc={acc} C={C} nblk={nblk}"
        names = ["dbeta"] + (["dgamma", "cA", "cB", "cC"] if bn else []) + (["dslope"] if want_slope else [])
        for k in names:
            add = pre[k] if (acc and k in pre) else 0.0
            assert_fp64_truth(f"{k} {tag}", out[k].cpu(), (r32[k] + add).double(), r64[k] + (add.double() if acc and k in pre else 0.0),
                              report)
        if not bn:                                               # bias-only mode writes none of the BatchNorm outputs
            for k in ("dgamma", "cA", "cB", "cC"):
                ref = pre[k] if (acc and k in pre) else None
                v = untouched[k].cpu()
                assert torch.equal(v, ref) if ref is not None else bool((v == G.SENTINEL).all()), f"{k} written in bias-only mode ({tag})"
    G.print_report(f"finalize on synthetic partials C={C} nblk={nblk}", report)


# ================================================================================================ grouped forms
@pytest.mark.parametrize("groups", [2, 3])
@pytest.mark.parametrize("C, R", [(16, 63), (128, 2305), (64, 288)])
def test_grouped_backward_vs_fp64(ops, groups, C, R):
    """sst_bwd_reduce_grp / sst_bwd_finalize_grp / sst_bwd_apply_grp against per-pass F.batch_norm autograd in fp64.  Pass k has mean k
    and scale 2^k, so a coefficient row taken from the wrong pass is a gross error; dgamma / dbeta sum over the passes."""
    report = []
    gamma, beta = params(groups + C, C)
    ys = [make_rows(10 * groups + C + k, R, C, "normal", k) for k in range(groups)]
    gen = torch.Generator().manual_seed(groups * C + R)
    ups = [torch.randn(R, C, generator=gen).double() for _ in range(groups)]
    pre = {k: torch.randn(C, generator=gen).float().double() for k in ("dgamma", "dbeta")}
    aff = [affine_of(y, gamma, beta) for y in ys]
    pins = [G.undecided_signs(y, a[2], a[3], G.bn_act(y, gamma, beta, 0.0, 0))[0] for y, a in zip(ys, aff)]
    r64 = [G.chain_grads(y, u, gamma, beta, 0.2, 1, torch.float64, pin=p) for y, u, p in zip(ys, ups, pins)]
    r32 = [G.chain_grads(y.float(), u.float(), gamma, beta, 0.2, 1, torch.float32, pin=p) for y, u, p in zip(ys, ups, pins)]
    mean, rstd, scale, shift = (dev(torch.stack([a[i] for a in aff])) for i in range(4))
    yd, ud = dev(torch.cat(ys)), dev(torch.cat(ups))
    for acc in (0, 1):
        gd = G.Guarded()
        with gd.patch(ops):
            part = ops.bwd_reduce(ud, yd, scale=scale, shift=shift, slope_const=0.2, act=1, groups=groups)
            assert part.shape[0] == groups * G.reduce_blocks(R, C)
            dgamma, dbeta = (gd.put(pre[k]) if acc else gd.empty(C) for k in ("dgamma", "dbeta"))
            cA, cB, cC = ops.bwd_finalize(part, R, mean, rstd, dev(gamma), dgamma, dbeta, accumulate=bool(acc), groups=groups)
            dy = ops.bwd_apply(ud, yd, scale=scale, shift=shift, slope_const=0.2, act=1, cA=cA, cB=cB, cC=cC, groups=groups)
        for k in range(groups):
            assert_fp64_truth(f"dy pass {k} of {groups} C={C} R={R}", dy[k * R:(k + 1) * R].cpu(), r32[k]["dy"].double(), r64[k]["dy"],
                              report)
        for name, h in (("dgamma", dgamma), ("dbeta", dbeta)):
            add = pre[name] if acc else 0.0
            assert_fp64_truth(f"{name} groups={groups} C={C} R={R} acc={acc}", h.cpu(),
                              (sum(r[name] for r in r32) + (add.float() if acc else 0.0)).double(), sum(r[name] for r in r64) + add, report)
    G.print_report(f"grouped backward groups={groups} C={C} R={R}", report)


# ================================================================================================ bwd_apply alone
def _apply_case(ops, R, C, seed, has_g2, act, affine):
    """dy = fmaf(cA, gz, fmaf(cB, y, cC)) with random coefficients.  k = 4: g + g2, gz = g * slope, the two fmaf."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    up, y = r(R, C), r(R, C)
    up2 = r(R, C) if has_g2 else None
    cA, cB, cC = r(C), r(C), r(C)
    scale, shift = (r(C), r(C)) if affine else (None, None)
    slope = 0.2
    with G.Guarded().patch(ops):
        dy = ops.bwd_apply(dev(up), dev(y), g2=dev(up2), scale=dev(scale), shift=dev(shift), slope_const=slope, act=act,
                           cA=dev(cA), cB=dev(cB), cC=dev(cC))
    d = lambda t: None if t is None else t.double()
    upt = d(up) if up2 is None else d(up) + d(up2)
    gz = G.bwd_gz(upt, d(y), d(scale), d(shift), float(torch.tensor(slope).float()), act)[0]
    ref = G.bwd_apply(gz, d(y), d(cA), d(cB), d(cC))
    terms = (d(cA) * gz).abs() + (d(cB) * d(y)).abs() + d(cC).abs()
    return dy, ref, terms


APPLY_CASES = [  # (C, R, fixed_c): grid_for(R*C/4) * 256 % (C/4) zero and non-zero for each channel count that can be either
    (12, 256, True), (12, 100, False), (12, 5000, False), (96, 32, True), (96, 11, False), (96, 690, False), (160, 32, True),
    (160, 7, False), (160, 333, False), (64, 1, True), (64, 50, True), (64, 4097, True)]


@pytest.mark.parametrize("C, R, expect", APPLY_CASES)
def test_bwd_apply_coefficient_reload(ops, C, R, expect):
    """The `!fixed_c` reload of scale / shift / cA / cB / cC (channel counts that are no power of two) against the once-loaded form."""
    fixed = G.apply_fixed_c(R, C)
    assert fixed == expect, "the case no longer takes the branch it was chosen for"
    for has_g2, act, affine in ((0, 1, 1), (1, 1, 0), (1, 0, 0)):
        dy, ref, terms = _apply_case(ops, R, C, 31 * C + R, has_g2, act, affine)
        G.assert_elementwise(f"bwd_apply C={C} R={R} fixed_c={fixed} g2={has_g2} act={act} affine={affine}", dy, ref, terms, 4)


def test_bwd_apply_branch_cases_cover_both():
    got = {}
    for C, R, expect in APPLY_CASES:
        assert G.apply_fixed_c(R, C) == expect
        got.setdefault(C, set()).add(expect)
    assert got == {12: {True, False}, 96: {True, False}, 160: {True, False}, 64: {True}}


STRIDE4 = 2048 * 256 * 4              # float4 items one sweep of the unrolled batch covers once the grid is capped


@pytest.mark.parametrize("C, R", [(4, STRIDE4 - 1), (4, STRIDE4), (4, STRIDE4 + 1), (12, 699050), (12, 699051), (64, STRIDE4 // 16),
                                  (64, STRIDE4 // 16 + 1)])
def test_bwd_apply_unrolled_batch_and_tail(ops, C, R):
    """total = R*C/4 one below, at and one above stride*4 (C = 4: one float4 per row, so `total` moves by one; C = 12: two below and
    one above, no fixed channel quad; C = 64: at and 16 above): the batch re-reads item i0 past the end and leaves with `break`."""
    total, s4 = R * (C // 4), STRIDE4
    assert G.grid_for(total, 2048) == 2048 and abs(total - s4) <= 16
    assert G.apply_fixed_c(R, C) == (C != 12)
    dy, ref, terms = _apply_case(ops, R, C, C + R % 1000, 1, 1, 1)
    G.assert_elementwise(f"bwd_apply C={C} R={R} total - stride*4 = {total - s4}", dy, ref, terms, 4)


@pytest.mark.parametrize("B, H, W, C", [(2, 8, 12, 64), (1, 2, 2, 4), (3, 6, 10, 16)])
def test_bwd_apply_unshuffle(ops, B, H, W, C):
    """unshuffle=True stores dy in the pre-PixelShuffle(2) layout: bit-equal to F.pixel_unshuffle of the plain store, whose values are
    held elementwise (k = 4 as above)."""
    gen = torch.Generator().manual_seed(B * H * W * C)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    up, y, up2, cA, cB, cC = r(B, H, W, C), r(B, H, W, C), r(B, H, W, C), r(C), r(C), r(C)
    sl = torch.tensor([0.25])
    with G.Guarded().patch(ops):
        kw = dict(g2=dev(up2), slope=dev(sl), act=1, cA=dev(cA), cB=dev(cB), cC=dev(cC))
        plain = ops.bwd_apply(dev(up), dev(y), **kw)
        uns = ops.bwd_apply(dev(up), dev(y), unshuffle=True, **kw)
        act_only = ops.bwd_apply(dev(up), dev(y), g2=dev(up2), slope=dev(sl), act=1, unshuffle=True)
    assert tuple(uns.shape) == (B, H // 2, W // 2, 4 * C)
    assert torch.equal(uns.cpu(), G.pixel_unshuffle_rows(plain.cpu().view(-1, C), B, H, W))
    d = lambda t: t.double().view(-1, t.shape[-1])
    gz = G.bwd_gz(d(up) + d(up2), d(y), None, None, 0.25, 1)[0]
    ref = G.bwd_apply(gz, d(y), cA.double(), cB.double(), cC.double())
    G.assert_elementwise("bwd_apply before the unshuffle store", plain.view(-1, C), ref,
                         (cA.double() * gz).abs() + (cB.double() * d(y)).abs() + cC.double().abs(), 4)
    G.assert_elementwise("activation-only unshuffle (k = 2: g + g2, * slope)", act_only,
                         G.pixel_unshuffle_rows(gz, B, H, W), G.pixel_unshuffle_rows(gz.abs(), B, H, W), 2)


# ================================================================================================ forward finalize
def _tile_counts(nt, seed):
    """Unequal tile counts 0..7 with empty tiles in the register path and, past 1024 tiles, in the plain loop (its first, one in the
    middle, its last); one tile of one row when nt == 1 (the n == 1 case of the unbiased running variance)."""
    if nt == 1:
        return [1]
    gen = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 8, (nt,), generator=gen)
    counts[0] = 5
    counts[min(3, nt - 1)] = 0
    if nt > 1024:
        counts[1024:] = torch.randint(1, 8, (nt - 1024,), generator=gen)
        for i in {1025, (1024 + nt) // 2, nt - 1} - {1024}:
            if i < nt:
                counts[i] = 0
    return counts.tolist()


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("C", [3, 64, 512])
@pytest.mark.parametrize("nt", [1, 7, 1024, 1025, 4608])
def test_bn_finalize_vs_fp64(ops, nt, C, groups):
    """sst_bn_finalize(_grp) on per-tile (sum, M2, count) built on the host from an fp64 tensor; nt tiles per group.  Truth: the
    statistics of the tensor itself in fp64; fp32 reference: Chan's combination of the same tiles in fp32 torch.  With running
    statistics (one momentum step per group, in order, unbiased variance) and without."""
    report = []
    gamma, beta = params(nt + C, C)
    gen = torch.Generator().manual_seed(nt * C + groups)
    rm0, rv0 = torch.randn(C, generator=gen).float(), (torch.rand(C, generator=gen) + 0.5).float()
    stats, cnts, passes = [], [], []
    for k in range(groups):
        counts = _tile_counts(nt, nt + C + k)
        y = make_rows(nt + C + k, int(sum(counts)), C, "normal", k)
        tid = torch.repeat_interleave(torch.arange(nt), torch.tensor(counts))
        y = (y + 2.0 ** k * torch.randn(nt, 1, generator=gen).double()[tid]).float().double()      # tile means apart: n_t d^2 matters
        s, c = G.make_tiles(y, counts)
        stats.append(s.float()), cnts.append(c.float()), passes.append(y)
    sd, cd = dev(torch.cat(stats)), dev(torch.cat(cnts))

    def refs(dtype):
        rm, rv, out = rm0.to(dtype), rv0.to(dtype), []
        for k in range(groups):
            if dtype == torch.float64:
                y = passes[k]
                n, mean, m2 = y.shape[0], y.mean(0), ((y - y.mean(0)) ** 2).sum(0)
            else:
                n, mean, m2 = G.chan_combine(stats[k], cnts[k])
            r = G.finalize_from(float(n), mean, m2, gamma.to(dtype), beta.to(dtype), rm, rv)
            rm, rv = r[4], r[5]
            out.append(r[:4])
        return [torch.stack([o[i] for o in out]) for i in range(4)] + [rm, rv]
    r64, r32 = refs(torch.float64), refs(torch.float32)
    for running in (True, False):
        gd = G.Guarded()
        rm, rv = (gd.put(rm0), gd.put(rv0)) if running else (None, None)
        with gd.patch(ops):
            got = list(ops.bn_finalize(sd, cd, dev(gamma), dev(beta), rm, rv, groups=groups))
        assert tuple(got[0].shape) == ((C,) if groups == 1 else (groups, C))
        names = ["mean", "rstd", "scale", "shift"] + (["run_mean", "run_var"] if running else [])
        for i, (name, h) in enumerate(zip(names, got + [rm, rv])):
            assert_fp64_truth(f"{name} nt={nt} C={C} groups={groups} running={running}", h.cpu().view(-1), r32[i].double().view(-1),
                              r64[i].view(-1), report)
    G.print_report(f"bn_finalize nt={nt} C={C} groups={groups}", report)


@pytest.mark.parametrize("C", [5, 64, 200])
@pytest.mark.parametrize("nrep", [1, 4])
def test_bn_finalize_acc_vs_fp64(ops, nrep, C):
    """sst_bn_finalize_acc on fp64 accumulators (sum, sum of squares) written from the host, rows spread over nrep replicas.  Channel 1
    is constant and its sum of squares sits four ulps below A*mean, as the rounding of the adds can leave it: Bq - A*mean is negative
    and must clamp to var = 0, rstd = 1/sqrt(eps)."""
    report = []
    n = 4 * 97
    y = make_rows(nrep * C, n, C, "normal")
    y[:, 1] = 0.3
    acc = torch.stack([torch.stack([p.sum(0), (p * p).sum(0)], 1) for p in y.chunk(nrep)])        # [nrep, C, 2]
    A = acc[:, 1, 0].sum()
    acc[:, 1, 1] = (A * (A / n)) * (1 - 4 * 2.0 ** -52) / nrep
    assert float(acc[:, 1, 1].sum() - A * (A / n)) < 0
    gamma, beta = params(nrep + C, C)
    gen = torch.Generator().manual_seed(nrep + C)
    rm0, rv0 = torch.randn(C, generator=gen).float(), (torch.rand(C, generator=gen) + 0.5).float()

    def refs(dtype):
        yy = y.to(dtype)
        mean = yy.mean(0)
        return G.finalize_from(float(n), mean, ((yy - mean) ** 2).sum(0), gamma.to(dtype), beta.to(dtype), rm0.to(dtype), rv0.to(dtype))
    r64, r32 = refs(torch.float64), refs(torch.float32)
    assert float(r64[1][1]) == pytest.approx(G.EPS ** -0.5, rel=1e-12)
    for running in (True, False):
        gd = G.Guarded()
        rm, rv = (gd.put(rm0), gd.put(rv0)) if running else (None, None)
        with gd.patch(ops):
            got = list(ops.bn_finalize_acc(acc.cuda(), n, dev(gamma), dev(beta), rm, rv))
        assert bool(torch.isfinite(torch.stack(got)).all())
        assert got[1][1].item() == pytest.approx(G.EPS ** -0.5, rel=4 * G.U24)
        names = ["mean", "rstd", "scale", "shift"] + (["run_mean", "run_var"] if running else [])
        for i, (name, h) in enumerate(zip(names, got + [rm, rv])):
            assert_fp64_truth(f"{name} nrep={nrep} C={C} running={running}", h.cpu(), r32[i].double(), r64[i], report)
    G.print_report(f"bn_finalize_acc nrep={nrep} C={C}", report)


# ================================================================================================ elementwise helpers
@pytest.mark.parametrize("C", [1, 5, 64, 200])
def test_bn_eval_affine(ops, C):
    """scale = gamma / sqrt(run_var + eps): k = 3 (add, sqrt, divide).  shift = beta - run_mean*scale: k = 5 on |beta| + |run_mean scale|
    (the three of scale, the product, the subtraction)."""
    gen = torch.Generator().manual_seed(C)
    gamma, beta, rm = (torch.randn(C, generator=gen).float() for _ in range(3))
    rv = (torch.rand(C, generator=gen) * 2).float()
    rv[0] = 0.0
    with G.Guarded().patch(ops):
        scale, shift = ops.bn_eval_affine(dev(gamma), dev(beta), dev(rm), dev(rv))
    s64, t64 = G.eval_affine(gamma.double(), beta.double(), rm.double(), rv.double(), float(torch.tensor(G.EPS).float()))
    G.assert_elementwise("bn_eval_affine scale", scale, s64, s64.abs(), 3)
    G.assert_elementwise("bn_eval_affine shift", shift, t64, beta.double().abs() + (rm.double() * s64).abs(), 5)


@pytest.mark.parametrize("C, R", [(4, 2048 * 256 + 37), (64, 2048 * 16 + 37), (256, 2048 * 4 + 5), (64, 3)])
def test_bn_residual_and_add(ops, C, R):
    """out = fmaf(y, scale, shift) + act(res), R beyond the 2048-workgroup grid stride.  k = 3: res*slope, the fmaf, the add.
    add: one IEEE addition per element, bit-equal to torch's."""
    gen = torch.Generator().manual_seed(C + R)
    y, res = torch.randn(R, C, generator=gen).float(), torch.randn(R, C, generator=gen).float()
    sc, sh = torch.randn(C, generator=gen).float(), torch.randn(C, generator=gen).float()
    sl = torch.tensor([0.3]).float()
    if R * (C // 4) > 256:
        assert G.grid_for(R * (C // 4), 2048) == 2048 and R * (C // 4) > 2048 * 256
    yd, rd = dev(y), dev(res)
    with G.Guarded().patch(ops):
        with_slope = ops.bn_residual(yd, dev(sc), dev(sh), rd, dev(sl))
        without = ops.bn_residual(yd, dev(sc), dev(sh), rd)
        added = ops.add(yd, rd)
    a = y.double() * sc.double() + sh.double()
    terms = (y.double() * sc.double()).abs() + sh.double().abs() + res.double().abs()
    G.assert_elementwise("bn_residual with slope", with_slope, a + G.slope_act(res.double(), sl.double()), terms, 3)
    G.assert_elementwise("bn_residual without slope", without, a + res.double(), terms, 3)
    assert torch.equal(added.cpu(), y + res)


# ================================================================================================ rejected arguments
def test_rejected_arguments(ops):
    """Each call must come back from SST_REQUIRE as HipPathError before any launch."""
    from srganst._abi import HipPathError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for C in (12, 2048):                                         # 256 % (C/4) != 0; more than 1024 channels
        with pytest.raises(HipPathError):
            ops.bwd_reduce(z(8, C), z(8, C))
    with pytest.raises(HipPathError):                            # C % 4 != 0
        ops.bwd_apply(z(8, 6), z(8, 6))
    with pytest.raises(HipPathError):                            # ntiles % groups != 0
        ops.bn_finalize(z(7, 2, 8), z(7), z(8), z(8), groups=2)
    for shape in ((1, 3, 4, 8), (1, 4, 5, 8)):                   # odd unshuffle geometry
        with pytest.raises(HipPathError):
            ops.bwd_apply(z(*shape), z(*shape), unshuffle=True)
    torch.cuda.synchronize()
