"""GPU: the discriminator's classifier kernels (csrc/linear.hip) held to plain torch fp64 on the CPU at the shapes where their tiles,
tails and branches change: flatten_act, the split-K linear_fwd + linear_reduce, linear_dgrad<MT> with its NHWC scatter, the FMA and
MFMA weight gradients, colsum_small, head_fwd and head_bwd.

Rules:
  integer data in [-3, 3]      bitwise (`exact` asserts on the CPU that every partial sum stays below 2^24 in its unit, so fp32 sums
                               are exact in any order and the HIP result must equal the fp64 reference bit for bit: an indexing test)
  random data                  norm-wise relative error below TOL = 2e-5 (tests/test_kernels_gpu.py: fp32 FMA / MFMA chains differ
                               from fp64 by re-association only)
  non-finite data              isnan / isinf masks equal to the fp64 reference's, the finite remainder within TOL
Every output - and linear_fwd's split-K slab - lives between two sentinel-filled guard bands of 4096 floats, checked after the
launches: out-of-range stores are caught without causing any.

Which branch of linear.hip a case reaches (M, N, K):
  linear_fwd     row tiles t = 0..3 by M = 1 / 15-17 / 32-33 / 48-49 / 63-64; `m < M` padding rows by M % 16 != 0; the `kk + 3 < ke`
                 scalar tails and misaligned 16-byte rows by K % 4 != 0 and by K < 16 (K = 1, 3, 67, 203, 1027); the `min(n0 + lj, N - 1)`
                 clamp by N = 1, 3, 13, 15, 17, 65, 130; more slabs sized than used by (16, 1024, 4100): ks = 16, 13 launched
  linear_reduce  bias / no bias; the grid stride by (64, 2064, 100): M N = 132096 > 512 * 256
  linear_dgrad   MT = 1..4 by M as above; main loop only where K >= 64 and a wave has 4 U rows (U = 8 at MT = 1, else 4): never at
                 N = 64 / MT = 1 (16 rows per wave), main + tail at N = 200 (waves of 52, 52, 52, 44 rows), main only at (32, 128, 64);
                 `nn < ne` in the last wave by N = 130 (22 rows), 17, 1, 3, 13; empty waves by N = 1, 3 (three) and 13 (one: 4, 4, 4, 1);
                 the partial last k block by K % 64 != 0, alone (K = 1, 3) and after full ones; with the scatter by K = 84, 125, 576
  linear_wgrad   the scalar path by K % 4 != 0; the float4 path by K % 4 == 0 with N % 64 != 0 or K % 32 != 0, and by
                 SST_LINEAR_WGRAD_FMA at MFMA shapes; `n0 + j >= N` by N % 16 != 0; the second k block by K = 1027, 4100, 18432
  wgrad_mfma     K % 32 == 0 and N % 64 == 0: (1,64,64) .. (64,64,96), (32,128,64), (64,1024,18432); odd M by 1, 15, 17, 33, 49, 63
                 (`m < M`); more than one batch of 8 row pairs by M > 16; `k0 >= K` by K = 64, 96 (a workgroup covers 128 columns)
  colsum_small   N = 1 .. 2064 (nine workgroups), write and accumulate
  head_fwd       N = 1, 2, 3, 64; K < 256 (idle threads), K % 256 != 0, K = 1
  head_bwd       M % 8 != 0, blockIdx.y > 0 by M >= 9, the second k block by K = 257 .. 1500, dw / db null, accumulate
  flatten_act    act on / off, affine on / off, grouped coefficients, the grid stride by 16 x 6 x 6 x 1024 = 589824 > 2048 * 256
Run with -s for the error tables."""
import pytest
import torch
import torch.nn.functional as F

import glue_refs as G
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
SLOPE_EXACT = 0.25                                               # a power of two: LeakyReLU of an integer stays exact
GUARD = 4096                                                     # floats on either side (a multiple of 4: 16-byte stores stay aligned)


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


def dev(t):
    return None if t is None else t.detach().to(torch.float32).contiguous().cuda()


class Guarded(G.Guarded):
    """glue_refs.Guarded with bands of 4096 floats."""

    def empty(self, *shape, dtype=torch.float32, fill=None):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        n = 1
        for s in shape:
            n *= int(s)
        buf = torch.full((n + 2 * GUARD,), G.SENTINEL, device=self.device, dtype=torch.float32)
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for i, (buf, n) in enumerate(self.bufs):
            assert bool((buf[:GUARD] == G.SENTINEL).all()), f"guard band before output {i} ({n} floats) was written"
            assert bool((buf[GUARD + n:] == G.SENTINEL).all()), f"guard band after output {i} ({n} floats) was written"
        self.bufs = []


def exact(nterms, add=0, unit=1.0):
    """Operands are integers in [-3, 3] (times `unit`, a power of two): a sum of `nterms` products plus `add` more integers of that
    size stays a multiple of unit below 2^24 unit, so every fp32 partial sum is exact whatever the order."""
    assert unit in (1.0, 0.25, 0.0625)
    assert 9 * nterms + 3 * add < 2 ** 24, f"{nterms} terms leave the exact range of fp32"


def ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).double()


def same(name, hip, ref64):
    hip = hip.detach().cpu()
    assert hip.dtype == torch.float32 and tuple(hip.shape) == tuple(ref64.shape), f"{name}: shape {tuple(hip.shape)} / {tuple(ref64.shape)}"
    if not torch.equal(hip.double(), ref64):
        bad = (hip.double() != ref64).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {ref64.numel()} elements differ from fp64, first at {bad[0].tolist()}: "
                             f"hip {hip[tuple(bad[0])].item()} ref {ref64[tuple(bad[0])].item()}")


def close(name, hip, ref64, report=None):
    e = rel_err(hip.detach().cpu(), ref64)
    if report is not None:
        report.append((name, e))
    assert e < TOL, f"{name}: |hip - fp64| / |fp64| = {e:.3e} >= {TOL}"


def show(title, report):
    print(f"\n{title}")
    for name, e in report:
        print(f"  {name:40s} {e:.3e}")


# ================================================================================================ references (fp64, CPU)
def linear_ref(x, w, b, dy):
    """y, dx, dw, db of F.linear by autograd in fp64."""
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    y = F.linear(x, w, b)
    y.backward(dy)
    return {"y": y.detach(), "y0": F.linear(x.detach(), w.detach()), "dx": x.grad, "dw": w.grad, "db": b.grad}


def scatter_ref(dx, C, HW):
    """dx [M, C*HW] in NCHW-flatten order -> NHWC [M, HW*C]."""
    M = dx.shape[0]
    return dx.view(M, C, HW).transpose(1, 2).contiguous().view(M, HW * C)


def head_ref(h, w, b, dy, slope):
    h, w = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    y = F.linear(F.leaky_relu(h, slope), w, b)
    y.backward(dy)
    return {"y": y.detach(), "y0": F.linear(F.leaky_relu(h.detach(), slope), w.detach()), "dh": h.grad, "dw": w.grad, "db": b.grad}


def flatten_ref(y, scale, shift, slope, act, grp=0):
    """y [B,H,W,C] -> act(y * scale + shift) as [B, C*H*W]; grp > 0: scale / shift [B / grp, C]."""
    B = y.shape[0]
    v = y
    if scale is not None:
        s = scale.view(-1, scale.shape[-1]).repeat_interleave(grp if grp else B, 0)
        t = shift.view(-1, shift.shape[-1]).repeat_interleave(grp if grp else B, 0)
        v = y * s.view(B, 1, 1, -1) + t.view(B, 1, 1, -1)
    if act:
        v = F.leaky_relu(v, slope)
    return v.permute(0, 3, 1, 2).flatten(1)


# ================================================================================================ cases
MT_CASES = [(1, 64, 64), (15, 64, 96), (16, 64, 96), (17, 64, 96), (32, 128, 64), (33, 64, 96), (48, 64, 64), (49, 64, 96), (63, 64, 96),
            (64, 64, 96)]
K_CASES = [(5, 24, 1), (5, 24, 3), (33, 40, 67), (64, 17, 203), (16, 130, 1027)]
DGRAD_CASES = [(1, 200, 200), (17, 200, 203), (16, 130, 128), (64, 130, 64), (3, 1, 64), (3, 3, 70), (3, 13, 64)]
SMALL_N_CASES = [(4, 1, 300), (4, 15, 300), (33, 65, 64)]
REDUCE_CASE = (64, 2064, 100)
SLAB_CASE = (16, 1024, 4100)
WORKLOAD = (64, 1024, 18432)
# beyond the issue's table: MT = 2 and 3 with a main loop AND a ragged tail (N = 200 at U = 4: 52 = 3 * 16 + 4, last wave 44 = 2 * 16 + 12)
# and K % 64 != 0; K below one MFMA step with a full row tile
EXTRA_CASES = [(32, 200, 70), (48, 130, 131), (16, 16, 2)]
LINEAR_CASES = MT_CASES + K_CASES + DGRAD_CASES + SMALL_N_CASES + [REDUCE_CASE, SLAB_CASE, WORKLOAD] + EXTRA_CASES
RAGGED_CASES = [c for c in LINEAR_CASES if c[0] % 16 or c[1] % 16 or c[2] % 64]

SCATTER_CASES = [(3, 12, 7, 24), (17, 64, 9, 130), (64, 25, 5, 64), (2, 512, 36, 1024)]                  # (M, C, HW, N)
HEAD_CASES = [(1, 1, 1), (7, 1, 255), (8, 3, 256), (9, 3, 257), (16, 1, 1024), (33, 64, 1500), (64, 2, 1024)]
FLATTEN_CASES = [(1, 1, 1, 1), (3, 3, 5, 8), (2, 6, 6, 512), (16, 6, 6, 1024)]                              # (B, H, W, C)


def fwd_slabs(M, N, K):
    """(slabs sized by sst_linear_ksplit, slabs one launch writes): linear.hip's own arithmetic, restated."""
    ks = max(1, 1024 // ((N + 15) // 16))
    while ks > 1 and K // ks < 256:
        ks >>= 1
    kslice = ((K + ks - 1) // ks + 63) // 64 * 64
    return ks, (K + kslice - 1) // kslice


def linear_data(case, integer):
    M, N, K = case
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + (0 if integer else 7))
    if integer:
        x, w, b, dy = ints(gen, M, K), ints(gen, N, K), ints(gen, N), ints(gen, M, N)
        pw, pb = ints(gen, N, K), ints(gen, N)
        exact(K, add=1), exact(N), exact(M, add=1)              # y (+ bias), dx, dw / db (+ what they accumulate onto)
    else:
        r = lambda *s: torch.randn(*s, generator=gen).float().double()
        x, w, b, dy = r(M, K), (r(N, K) / K ** 0.5).float().double(), r(N), r(M, N)
        pw, pb = r(N, K), r(N)
    return x, w, b, dy, pw, pb


def run_linear(ops, x, w, b, dy, pw, pb, nhwc=None):
    """Every op of the linear layer once, all outputs (and the slab) between guard bands; returns host copies."""
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    N, K = w.shape
    gd = Guarded()
    with gd.patch(ops):
        out = {"y": ops.linear_fwd(xd, wd, bd), "y0": ops.linear_fwd(xd, wd, None), "dx": ops.linear_dgrad(dyd, wd, nhwc=nhwc)}
        out["dw"], out["db"] = gd.empty(N, K), gd.empty(N)
        ops.linear_wgrad(dyd, xd, out["dw"], out["db"])
        out["dw_acc"], out["db_acc"] = gd.put(pw), gd.put(pb)
        ops.linear_wgrad(dyd, xd, out["dw_acc"], out["db_acc"], accumulate=True)
        out["dw_only"] = gd.empty(N, K)
        ops.linear_wgrad(dyd, xd, out["dw_only"], None)
    return {k: v.cpu() for k, v in out.items()}


def check_linear(tag, got, ref, pw, pb, cmp, nhwc=None):
    dx = scatter_ref(ref["dx"], *nhwc) if nhwc else ref["dx"]
    cmp(f"y {tag}", got["y"], ref["y"])
    cmp(f"y without bias {tag}", got["y0"], ref["y0"])
    cmp(f"dx {tag}", got["dx"], dx)
    cmp(f"dw {tag}", got["dw"], ref["dw"])
    cmp(f"db {tag}", got["db"], ref["db"])
    cmp(f"dw accumulated {tag}", got["dw_acc"], pw + ref["dw"])
    cmp(f"db accumulated {tag}", got["db_acc"], pb + ref["db"])
    assert torch.equal(got["dw_only"], got["dw"]), f"dw without db differs from dw with db ({tag})"


# ================================================================================================ 1. exact integers
def test_case_table_reaches_the_branches():
    """The shape arithmetic the table above relies on, restated from linear.hip: if a launcher changes, the cases must be re-chosen."""
    assert fwd_slabs(*SLAB_CASE) == (16, 13) and fwd_slabs(*WORKLOAD) == (16, 16) and fwd_slabs(4, 1, 300) == (1, 1)
    assert REDUCE_CASE[0] * REDUCE_CASE[1] > 512 * 256
    assert {(m + 15) // 16 for m, _, _ in LINEAR_CASES} == {1, 2, 3, 4}
    nper = lambda N: ((N + 3) // 4 + 3) // 4 * 4
    assert nper(200) == 52 and nper(130) == 36 and nper(13) == 4 and nper(64) == 16 and nper(3) == 4
    assert FLATTEN_CASES[-1][0] * 36 * 1024 > 2048 * 256
    assert all(c in RAGGED_CASES for c in K_CASES + SMALL_N_CASES + [REDUCE_CASE, SLAB_CASE]) and WORKLOAD not in RAGGED_CASES


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_linear_exact_on_integers(ops, case):
    """fwd with and without bias, dgrad, wgrad + db written and accumulated onto a non-zero integer gradient: bit-equal to fp64."""
    x, w, b, dy, pw, pb = linear_data(case, integer=True)
    got = run_linear(ops, x, w, b, dy, pw, pb)
    check_linear(str(case), got, linear_ref(x, w, b, dy), pw, pb, same)


@pytest.mark.parametrize("case", SCATTER_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dgrad_nhwc_scatter_exact_on_integers(ops, case):
    """dx scattered from the NCHW-flatten index k = c HW + hw to NHWC [M, HW, C], against the permuted fp64 product, and
    bit-equal to the permuted plain store."""
    M, C, HW, N = case
    K = C * HW
    gen = torch.Generator().manual_seed(M + C + HW + N)
    w, dy = ints(gen, N, K), ints(gen, M, N)
    exact(N)
    gd = Guarded()
    with gd.patch(ops):
        nhwc = ops.linear_dgrad(dev(dy), dev(w), nhwc=(C, HW))
        plain = ops.linear_dgrad(dev(dy), dev(w))
    same(f"dx NHWC {case}", nhwc, scatter_ref(dy @ w, C, HW))
    same(f"dx {case}", plain, dy @ w)


def head_data(case, integer):
    M, N, K = case
    gen = torch.Generator().manual_seed(7919 * M + 101 * N + K + (0 if integer else 7))
    if integer:
        h, w, b, dy, pw, pb = ints(gen, M, K), ints(gen, N, K), ints(gen, N), ints(gen, M, N), ints(gen, N, K), ints(gen, N)
        exact(K, add=1, unit=0.25), exact(N, unit=0.25), exact(M, add=1, unit=0.25)
        return h, w, b, dy, pw, pb, SLOPE_EXACT
    r = lambda *s: torch.randn(*s, generator=gen).float().double()
    return r(M, K), (r(N, K) / K ** 0.5).float().double(), r(N), r(M, N), r(N, K), r(N), 0.2


def run_head(ops, h, w, b, dy, pw, pb, slope):
    hd, wd, bd, dyd = dev(h), dev(w), dev(b), dev(dy)
    N, K = w.shape
    gd = Guarded()
    with gd.patch(ops):
        out = {"y": ops.head_fwd(hd, wd, bd, slope), "y0": ops.head_fwd(hd, wd, None, slope)}
        out["dw"], out["db"] = gd.empty(N, K), gd.empty(N)
        out["dh"] = ops.head_bwd(hd, wd, dyd, slope, out["dw"], out["db"])
        out["dh_only"] = ops.head_bwd(hd, wd, dyd, slope)
        out["dw_acc"], out["db_acc"] = gd.put(pw), gd.put(pb)
        out["dh_acc"] = ops.head_bwd(hd, wd, dyd, slope, out["dw_acc"], out["db_acc"], accumulate=True)
        out["dw_only"], out["db_only"] = gd.empty(N, K), gd.empty(N)
        out["dh_dw"] = ops.head_bwd(hd, wd, dyd, slope, out["dw_only"], None)
        out["dh_db"] = ops.head_bwd(hd, wd, dyd, slope, None, out["db_only"])
    return {k: v.cpu() for k, v in out.items()}


def check_head(tag, got, ref, pw, pb, cmp):
    cmp(f"head y {tag}", got["y"], ref["y"])
    cmp(f"head y without bias {tag}", got["y0"], ref["y0"])
    cmp(f"head dh {tag}", got["dh"], ref["dh"])
    cmp(f"head dw {tag}", got["dw"], ref["dw"])
    cmp(f"head db {tag}", got["db"], ref["db"])
    cmp(f"head dw accumulated {tag}", got["dw_acc"], pw + ref["dw"])
    cmp(f"head db accumulated {tag}", got["db_acc"], pb + ref["db"])
    for k in ("dh_only", "dh_acc", "dh_dw", "dh_db"):
        assert torch.equal(got[k], got["dh"]), f"head dh changes with dw / db / accumulate ({k}, {tag})"
    assert torch.equal(got["dw_only"], got["dw"]) and torch.equal(got["db_only"], got["db"]), f"head dw / db alone differ ({tag})"


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_exact_on_integers(ops, case):
    """head_fwd with and without bias; head_bwd's dh / dw / db, with dw and db null (dh unchanged), with either alone, and
    accumulated onto non-zero integers; slope 0.25 keeps LeakyReLU and its derivative exact (h = 0 takes the slope, as torch does)."""
    h, w, b, dy, pw, pb, slope = head_data(case, integer=True)
    got = run_head(ops, h, w, b, dy, pw, pb, slope)
    check_head(str(case), got, head_ref(h, w, b, dy, slope), pw, pb, same)


# ================================================================================================ 2. random data
@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_linear_random_vs_fp64(ops, case):
    """The same calls on normal data (w ~ 1 / sqrt(K)) within TOL of fp64; a second run of every op is bit-identical (no atomics)."""
    report = []
    x, w, b, dy, pw, pb = linear_data(case, integer=False)
    got = run_linear(ops, x, w, b, dy, pw, pb)
    check_linear(str(case), got, linear_ref(x, w, b, dy), pw, pb, lambda n, h, r: close(n, h, r, report))
    again = run_linear(ops, x, w, b, dy, pw, pb)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: second launch differs ({case})"
    show(f"linear {case}", report)


@pytest.mark.parametrize("case", SCATTER_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dgrad_nhwc_scatter_random_vs_fp64(ops, case):
    M, C, HW, N = case
    K = C * HW
    gen = torch.Generator().manual_seed(M + C + HW + N + 7)
    w = (torch.randn(N, K, generator=gen) / N ** 0.5).double()
    dy = torch.randn(M, N, generator=gen).double()
    gd = Guarded()
    with gd.patch(ops):
        nhwc = ops.linear_dgrad(dev(dy), dev(w), nhwc=(C, HW)).cpu()
        plain = ops.linear_dgrad(dev(dy), dev(w)).cpu()
        again = ops.linear_dgrad(dev(dy), dev(w), nhwc=(C, HW)).cpu()
    close(f"dx NHWC {case}", nhwc, scatter_ref(dy @ w, C, HW))
    assert torch.equal(nhwc, scatter_ref(plain, C, HW)), "the scatter changes values, not only places"
    assert torch.equal(nhwc, again), "second launch differs"


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_random_vs_fp64(ops, case):
    report = []
    h, w, b, dy, pw, pb, slope = head_data(case, integer=False)
    got = run_head(ops, h, w, b, dy, pw, pb, slope)
    check_head(str(case), got, head_ref(h, w, b, dy, float(torch.tensor(slope).float())), pw, pb, lambda n, hp, r: close(n, hp, r, report))
    again = run_head(ops, h, w, b, dy, pw, pb, slope)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: second launch differs ({case})"
    show(f"head {case}", report)


# ================================================================================================ 3. the slab, straight through the C ABI
@pytest.mark.parametrize("case", RAGGED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fwd_slab_of_exact_size(ops, case):
    """sst_linear_fwd with y and a slab of exactly sst_linear_ksplit(M, N, K) * M * N floats, both between guard bands: the bands stay
    untouched, y is the product, the slabs the launch used sum to it and the slabs it did not use still hold the sentinel."""
    from srganst import _abi
    from srganst._abi import check, ptr, stream_ptr
    M, N, K = case
    x, w, b, _, _, _ = linear_data(case, integer=True)
    ks, used = fwd_slabs(M, N, K)
    assert _abi.lib().sst_linear_ksplit(M, N, K) == ks
    xd, wd, bd = dev(x), dev(w), dev(b)
    gd = Guarded()
    y, slab = gd.empty(M, N), gd.empty(ks * M * N)
    check(_abi.lib().sst_linear_fwd(ptr(xd), ptr(wd), ptr(bd), ptr(y), ptr(slab), M, N, K, stream_ptr()), "sst_linear_fwd")
    y, slab = y.clone(), slab.clone().view(ks, M, N)
    gd.check()
    ref = F.linear(x, w, b)
    same(f"y {case}", y, ref)
    same(f"sum of the {used} slabs written {case}", slab[:used].sum(0), ref - b)
    assert bool((slab[used:] == G.SENTINEL).all()), f"a slab beyond the {used} launched was written ({case})"


# ================================================================================================ 4. kernel against kernel
@pytest.mark.parametrize("case", [(16, 64, 96), (33, 128, 64), (64, 1024, 1024)], ids=lambda c: "x".join(map(str, c)))
def test_wgrad_fma_against_mfma(ops, case, monkeypatch):
    """SST_LINEAR_WGRAD_FMA=1 (the FMA kernel at shapes the MFMA kernel takes by default): both bit-equal to fp64 and to each other
    on integers, both within TOL on random data, written and accumulated."""
    M, N, K = case
    assert K % 32 == 0 and N % 64 == 0
    for integer in (True, False):
        x, w, b, dy, pw, pb = linear_data(case, integer)
        ref = linear_ref(x, w, b, dy)
        runs = {}
        for name in ("mfma", "fma"):
            if name == "fma":
                monkeypatch.setenv("SST_LINEAR_WGRAD_FMA", "1")
            else:
                monkeypatch.delenv("SST_LINEAR_WGRAD_FMA", raising=False)
            gd = Guarded()
            dw, db, dwa, dba = gd.empty(N, K), gd.empty(N), gd.put(pw), gd.put(pb)
            ops.linear_wgrad(dev(dy), dev(x), dw, db)
            ops.linear_wgrad(dev(dy), dev(x), dwa, dba, accumulate=True)
            runs[name] = {"dw": dw.clone(), "db": db.clone(), "dw accumulated": dwa.clone(), "db accumulated": dba.clone()}
            gd.check()
        monkeypatch.delenv("SST_LINEAR_WGRAD_FMA", raising=False)
        want = {"dw": ref["dw"], "db": ref["db"], "dw accumulated": pw + ref["dw"], "db accumulated": pb + ref["db"]}
        for name, got in runs.items():
            for k, v in got.items():
                (same if integer else close)(f"{k} {name} {case}", v, want[k])
        if integer:
            for k in want:
                assert torch.equal(runs["mfma"][k], runs["fma"][k]), f"{k}: FMA and MFMA kernels differ on integers ({case})"


@pytest.mark.parametrize("N, K", [(130, 203), (1024, 4100), (24, 600)])
def test_rows_are_independent(ops, N, K):
    """Row m of a 64-row call equals the one-row call on that row, bit for bit, for linear_fwd (the split-K schedule ignores M),
    linear_dgrad (a wave's sum over n runs in the same order for every MT; only the load batching differs), head_fwd and head_bwd's
    dh; likewise within one row tile (M = 16) and across tiles (M = 17, 49)."""
    gen = torch.Generator().manual_seed(N + K)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    x, w, b, dy = r(64, K), r(N, K) / K ** 0.5, r(N), r(64, N)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    rows = (0, 15, 16, 47, 63)
    gd = Guarded()
    with gd.patch(ops):
        full = {"y": ops.linear_fwd(xd, wd, bd).cpu(), "dx": ops.linear_dgrad(dyd, wd).cpu()}
        for M in (16, 17, 49):
            assert torch.equal(ops.linear_fwd(xd[:M].contiguous(), wd, bd).cpu(), full["y"][:M]), f"linear_fwd: M={M} against M=64"
            assert torch.equal(ops.linear_dgrad(dyd[:M].contiguous(), wd).cpu(), full["dx"][:M]), f"linear_dgrad: M={M} against M=64"
        for m in rows:
            assert torch.equal(ops.linear_fwd(xd[m:m + 1].contiguous(), wd, bd).cpu()[0], full["y"][m]), f"linear_fwd row {m}"
            assert torch.equal(ops.linear_dgrad(dyd[m:m + 1].contiguous(), wd).cpu()[0], full["dx"][m]), f"linear_dgrad row {m}"
        if N <= 64:
            hy = ops.head_fwd(xd, wd, bd, 0.2).cpu()
            dh = ops.head_bwd(xd, wd, dyd, 0.2).cpu()
            for m in rows:
                assert torch.equal(ops.head_fwd(xd[m:m + 1].contiguous(), wd, bd, 0.2).cpu()[0], hy[m]), f"head_fwd row {m}"
                assert torch.equal(ops.head_bwd(xd[m:m + 1].contiguous(), wd, dyd[m:m + 1].contiguous(), 0.2).cpu()[0], dh[m]), f"head_bwd row {m}"


# ================================================================================================ 5. non-finite inputs
NONFINITE = [("row", float("nan")), ("row", float("inf")), ("row", float("-inf")), ("w", float("nan")), ("w", float("inf")),
             ("w", float("-inf")), ("lastcol", float("nan"))]


def poison(where, v, x, w, dy):
    """row: the last batch row (the one next to the padding rows) of x and dy, at its first, a middle and its last column; w: one
    element of the weight; lastcol: the last valid column N - 1 (the one the forward's clamp duplicates, the last the dgrad's ragged
    wave reads), in w's last row, at its last k, and in dy's first row."""
    x, w, dy = x.clone(), w.clone(), dy.clone()
    M, K = x.shape
    N = w.shape[0]
    if where == "row":
        x[M - 1, [0, K // 2, K - 1]] = v
        dy[M - 1, [0, N // 2, N - 1]] = v
    elif where == "w":
        w[N // 2, K // 3] = v
    else:
        w[N - 1, K - 1] = v
        dy[0, N - 1] = v
    return x, w, dy


def same_nonfinite(name, hip, ref64):
    hip = hip.detach().cpu()
    assert torch.equal(torch.isnan(hip), torch.isnan(ref64)), \
        f"{name}: NaN mask differs ({int(torch.isnan(hip).sum())} hip / {int(torch.isnan(ref64).sum())} fp64 of {hip.numel()})"
    assert torch.equal(torch.isposinf(hip), torch.isposinf(ref64)) and torch.equal(torch.isneginf(hip), torch.isneginf(ref64)), \
        f"{name}: inf mask differs"
    ok = torch.isfinite(ref64)
    if bool(ok.any()):
        e = rel_err(hip[ok], ref64[ok])
        assert e < TOL, f"{name}: finite remainder {e:.3e} >= {TOL}"


@pytest.mark.parametrize("where, v", NONFINITE, ids=lambda p: str(p))
@pytest.mark.parametrize("case", [(17, 24, 67), (49, 130, 200)], ids=lambda c: "x".join(map(str, c)))
def test_nonfinite_follows_torch(ops, case, where, v):
    """NaN / +inf / -inf in one row of x / dy / h, in one element of w, and NaN in the last valid column: the HIP outputs are NaN
    and +-inf exactly where the fp64 reference on the same data is, and within TOL elsewhere: padding rows (m >= M), clamped columns
    and zero-filled tails leak nothing into a valid output.  The head runs at N = min(N, 3)."""
    x0, w0, b, dy0, pw, pb = linear_data(case, integer=False)
    x, w, dy = poison(where, v, x0, w0, dy0)
    with torch.no_grad():
        ref = {"y": F.linear(x, w, b), "dx": dy @ w, "dw": dy.t() @ x, "db": dy.sum(0)}
    assert not all(bool(torch.isfinite(r).all()) for r in ref.values())
    got = run_linear(ops, x, w, b, dy, pw, pb)
    for k in ("y", "dx", "dw", "db"):
        same_nonfinite(f"{k} {case} {where} {v}", got[k], ref[k])
    same_nonfinite(f"dw accumulated {case} {where} {v}", got["dw_acc"], pw + ref["dw"])
    same_nonfinite(f"db accumulated {case} {where} {v}", got["db_acc"], pb + ref["db"])

    Nh = min(case[1], 3)
    h, hw, hdy = poison(where, v, x0, w0[:Nh], dy0[:, :Nh])
    hb, hpw, hpb = b[:Nh], pw[:Nh], pb[:Nh]
    slope = float(torch.tensor(0.2).float())
    href = head_ref(h, hw, hb, hdy, slope)
    hgot = run_head(ops, h, hw, hb, hdy, hpw, hpb, 0.2)
    for k in ("y", "dh", "dw", "db"):
        same_nonfinite(f"head {k} {case} {where} {v}", hgot[k], href[k])
    same_nonfinite(f"head dw accumulated {case} {where} {v}", hgot["dw_acc"], hpw + href["dw"])


# ================================================================================================ 6. flatten_act
@pytest.mark.parametrize("case", FLATTEN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_flatten_act(ops, case):
    """NHWC -> NCHW-flatten with act(y * scale + shift): affine + LeakyReLU, affine alone, LeakyReLU alone, neither (a pure
    permutation: bit-equal on random data), and B / 2 images per coefficient row where B is even.  Integers with slope 0.25: bit-equal
    to fp64.  Random data: rtol = atol = 1e-6 per element against fp64, as tests/test_discriminator_gpu.py holds the same kernel."""
    B, H, W, C = case
    gen = torch.Generator().manual_seed(B * H * W * C)
    variants = [(1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)] + ([(1, 1, B // 2), (1, 0, B // 2)] if B % 2 == 0 else [])
    for integer in (True, False):
        draw = (lambda *s: ints(gen, *s)) if integer else (lambda *s: torch.randn(*s, generator=gen).float().double())
        y = draw(B, H, W, C)
        slope = SLOPE_EXACT if integer else 0.2
        if integer:
            exact(1, add=1, unit=0.25)
        yd = dev(y)
        for affine, act, grp in variants:
            rows = (B // grp,) if grp else ()
            scale, shift = (draw(*rows, C), draw(*rows, C)) if affine else (None, None)
            gd = Guarded()
            with gd.patch(ops):
                flat = ops.flatten_act(yd, dev(scale), dev(shift), slope, act, grp=grp).cpu()
                out = gd.empty(B, C * H * W)
                assert ops.flatten_act(yd, dev(scale), dev(shift), slope, act, grp=grp, out=out) is out
                assert torch.equal(out.cpu(), flat), "second launch (into out=) differs"
            ref = flatten_ref(y, scale, shift, float(torch.tensor(slope).float()), act, grp)
            tag = f"flatten {case} affine={affine} act={act} grp={grp} {'integers' if integer else 'random'}"
            if integer or not (affine or act):
                same(tag, flat, ref)
            else:
                assert torch.allclose(flat.double(), ref, rtol=1e-6, atol=1e-6), f"{tag}: max abs err {float((flat.double() - ref).abs().max()):.3e}"


# ================================================================================================ 7. rejected arguments
def test_rejected_arguments(ops):
    """Each call must come back from SST_REQUIRE as HipPathError before any launch; the library stays usable afterwards."""
    from srganst import _abi
    from srganst._abi import HipPathError, ptr, stream_ptr
    z = lambda *s: torch.zeros(*s, device="cuda")
    L = _abi.lib()
    with pytest.raises(HipPathError):                            # M > 64
        ops.linear_fwd(z(65, 32), z(16, 32), z(16))
    with pytest.raises(HipPathError):
        ops.linear_dgrad(z(65, 16), z(16, 32))
    with pytest.raises(HipPathError):
        ops.linear_wgrad(z(65, 16), z(65, 32), z(16, 32), z(16))
    for nhwc in ((4, 7), (8, 5), (0, 32)):                       # C * HW != K = 32
        with pytest.raises(HipPathError):
            ops.linear_dgrad(z(3, 16), z(16, 32), nhwc=nhwc)
    with pytest.raises(HipPathError):                            # head: N > 64
        ops.head_fwd(z(4, 32), z(65, 32), z(65), 0.2)
    with pytest.raises(HipPathError):
        ops.head_bwd(z(4, 32), z(65, 32), z(4, 65), 0.2)
    with pytest.raises(HipPathError):                            # only one of scale / shift
        ops.flatten_act(z(2, 3, 3, 8), z(8), None, 0.2)
    with pytest.raises(HipPathError):
        ops.flatten_act(z(2, 3, 3, 8), None, z(8), 0.2)
    for grp in (3, 4, -1):                                       # grp does not divide B; negative
        with pytest.raises(HipPathError):
            ops.flatten_act(z(2, 3, 3, 8), z(2, 8), z(2, 8), 0.2, grp=grp)
    # null pointers and empty extents, straight through the C ABI (the wrappers cannot form them)
    a, w, y, s = z(4, 32), z(16, 32), z(4, 16), z(4 * 16)
    bad = [
        lambda: L.sst_linear_fwd(None, ptr(w), None, ptr(y), ptr(s), 4, 16, 32, stream_ptr()),
        lambda: L.sst_linear_fwd(ptr(a), ptr(w), None, ptr(y), None, 4, 16, 32, stream_ptr()),
        lambda: L.sst_linear_fwd(ptr(a), ptr(w), None, ptr(y), ptr(s), 0, 16, 32, stream_ptr()),
        lambda: L.sst_linear_fwd(ptr(a), ptr(w), None, ptr(y), ptr(s), 4, 0, 32, stream_ptr()),
        lambda: L.sst_linear_fwd(ptr(a), ptr(w), None, ptr(y), ptr(s), 4, 16, 0, stream_ptr()),
        lambda: L.sst_linear_dgrad(ptr(y), ptr(w), None, 4, 16, 32, 0, 0, stream_ptr()),
        lambda: L.sst_linear_dgrad(ptr(y), ptr(w), ptr(a), 0, 16, 32, 0, 0, stream_ptr()),
        lambda: L.sst_linear_wgrad(ptr(y), ptr(a), None, None, 4, 16, 32, 0, stream_ptr()),
        lambda: L.sst_linear_wgrad(ptr(y), ptr(a), ptr(w), None, 4, 16, 0, 0, stream_ptr()),
        lambda: L.sst_head_fwd(ptr(a), ptr(w), None, None, 4, 16, 32, 0.2, stream_ptr()),
        lambda: L.sst_head_fwd(ptr(a), ptr(w), None, ptr(y), 4, 0, 32, 0.2, stream_ptr()),
        lambda: L.sst_head_bwd(ptr(a), ptr(w), ptr(y), None, None, None, 4, 16, 32, 0.2, 0, stream_ptr()),
        lambda: L.sst_head_bwd(ptr(a), ptr(w), ptr(y), ptr(a), None, None, 0, 16, 32, 0.2, 0, stream_ptr()),
        lambda: L.sst_flatten_act_grp(ptr(a), None, None, 0.2, 1, None, 4, 4, 8, 0, stream_ptr()),
        lambda: L.sst_flatten_act_grp(ptr(a), None, None, 0.2, 1, ptr(a), 4, 0, 8, 0, stream_ptr()),
    ]
    for i, call in enumerate(bad):
        assert call() != 0, f"bad call {i} was accepted"
    torch.cuda.synchronize()
    # a good call of every entry point afterwards
    gen = torch.Generator().manual_seed(5)
    x, w, b, dy = ints(gen, 5, 24), ints(gen, 3, 24), ints(gen, 3), ints(gen, 5, 3)
    got = run_linear(ops, x, w, b, dy, w, b)
    check_linear("after the rejections", got, linear_ref(x, w, b, dy), w, b, same)
    hgot = run_head(ops, x, w, b, dy, w, b, SLOPE_EXACT)
    check_head("after the rejections", hgot, head_ref(x, w, b, dy, SLOPE_EXACT), w, b, same)
    yy = ints(gen, 2, 2, 3, 4)
    same("flatten after the rejections", ops.flatten_act(dev(yy), None, None, 0.2, 0), flatten_ref(yy, None, None, 0.2, 0))
