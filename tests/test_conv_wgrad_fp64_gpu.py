"""GPU: the weight-gradient kernels of csrc/conv_wgrad.hip (conv_wgrad_tile_kernel, conv_wgrad_band_kernel, conv_wgrad_kernel, the two
3-channel kernels, the slab reduces and the grouped entry) held to plain torch fp64 on the CPU at every launch plan and launch form.
The cases, the fp64 reference `wgrad64` and the restated plans live in tests/wgrad_refs.py; tests/test_wgrad_refs.py establishes on
the CPU that every case reaches the branch it was chosen for, so nothing here passes because its shape stopped reaching a kernel.

Rules (those of tests/test_conv_nsplit_fp64_gpu.py):
  integer data    x, dy and any dW accumulated onto in [-3, 3], scales in {0.5, 1, 2}, non-zero integer shifts in [-3, 3] (padding that is
                  not zeroed after the affine shows up), slope 0.25 (-1.5 for the select form): every term is a multiple of 1/8 (of 1
                  without affine) and `exact(terms64.max() + 3, unit)` asserts on the CPU that the sums stay below 2^24 units, so fp32 is
                  exact in any order and dW must equal fp64 bit for bit, written and accumulated.  This is the indexing test.
  random data     norm-wise |hip - fp64| / |fp64| < TOL = 2e-5, and elementwise |hip - fp64| <= k 2^-24 terms64 (+ |base| when
                  accumulating) with k = P + 8, P = B Ho Wo the products of one element's chain: chunk partials and the slab reduce are
                  re-associations of that chain, the 8 cover the affine FMA, the slope multiply and the accumulate add.  The inputs are
                  fp32 values, so the sign of every fmaf(x, scale, shift) is the fp64 sign: glue_refs.undecided_signs finds no
                  undecided activation branch.
  poison, guards  every launch goes through sst_conv_wgrad_grp / sst_conv_wgrad_grouped with a slab of exactly sst_conv_wgrad_chunks2
                  chunks pre-filled with NaN and a dW (NaN in write mode) from glue_refs.Guarded: a slab element the reduce reads and no
                  workgroup wrote, or a dW element never stored, fails the finiteness check; the chunks the plan writes must be finite
                  and the rest of the slab still NaN; stores outside either buffer fail Guarded.check().
  route           the kernel name is asserted before the launch; every launch is issued twice and compared with torch.equal.
Forms per case: plain; input affine + LeakyReLU(0.25) with the slope as a constant and read from the device (bit-equal); affine + slope
-1.5 from the device (the select form); each writing, accumulating, and with accumulate bit 2 followed by ops.wgrad_reduce_flush
(writing and accumulating; before the flush dW is untouched).  The 3-channel kernels take no affine and run plain.

Worst elementwise ratio |hip - fp64| / (2^-24 terms) seen on the MI355X, plain / affine / select (a record, not a threshold; the
threshold is k = P + 8, P from 60 to 230,400):
  tile    <2, 2, 8, 8> 1.83 / 2.06 / 1.76   <2, 2, 6, 8> 1.38 / 1.49 / 1.47   <1, 4, 8, 8> 0.71 / 0.59 / 0.56   <1, 4, 6, 8> 2.01 / 2.10 / 1.65
  band    <7> 1.36 / 1.50 / 1.16   <10> 1.61 / 2.12 / 1.82   grouped <7> (40 jobs) 1.92 plain, 1.91 with coefficients
  per-tap <true> 4.16 / 6.52 / 3.76   <false> 2.68 / 3.52 / 2.79   grouped <true> 2.09 plain, 2.56 with coefficients
  3-channel wgrad_k3c3_mfma_kernel 0.71   wgrad_k3c3_kernel 0.92          norm-wise 8.8e-8 .. 4.7e-7 over all cases
k is the worst case of the chain (every rounding in the same direction); on random data the roundings mostly cancel.
Run with -s for the tables."""
import ctypes
import struct

import pytest
import torch

import glue_refs as G
import wgrad_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
NAN = float("nan")
DATA = [True, False]
DATA_IDS = ["integers", "random"]
# launch form -> (form of the truth, slope read from the device)
LAUNCH_FORMS = {"plain": ("plain", False), "affine": ("affine", False), "affine slope-dev": ("affine", True), "select slope-dev": ("select", True)}
MODES = {"write": 0, "accumulate": 1, "deferred": 4, "deferred accumulate": 5}        # the `accumulate` argument of sst_conv_wgrad_grp


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


@pytest.fixture(scope="module")
def worst():
    """kernel name -> form -> worst elementwise ratio of the module's run; printed at the end (-s)."""
    table = {}
    yield table
    print("\n[conv_wgrad] worst |hip - fp64| / (2^-24 terms) per kernel, by form")
    for name, forms in sorted(table.items()):
        print(f"  {name:40s} " + "   ".join(f"{f} {v:.2f}" for f, v in sorted(forms.items())))


def note(worst, name, form, ratio):
    worst.setdefault(name, {})[form] = max(ratio, worst.get(name, {}).get(form, 0.0))


def dev(t):
    return None if t is None else t.detach().to(torch.float32).contiguous().cuda()


def same(name, hip, ref64):
    hip = hip.detach().cpu()
    assert hip.dtype == torch.float32 and tuple(hip.shape) == tuple(ref64.shape), f"{name}: shape {tuple(hip.shape)} / {tuple(ref64.shape)}"
    if not torch.equal(hip.double(), ref64):
        bad = (hip.double() != ref64).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {ref64.numel()} elements differ from fp64, first at {bad[0].tolist()}: "
                             f"hip {hip[tuple(bad[0])].item()} ref {ref64[tuple(bad[0])].item()}")


def held(name, hip, ref64, terms64, k, integer):
    """Integer data: bit-equal.  Random data: norm-wise and elementwise; -> (norm-wise error, worst elementwise ratio)."""
    if integer:
        same(name, hip, ref64)
        return 0.0, 0.0
    ratio = G.assert_elementwise(name, hip, ref64, terms64, k)
    e = rel_err(hip.detach().cpu(), ref64)
    assert e < TOL, f"{name}: |hip - fp64| / |fp64| = {e:.3e} >= {TOL}"
    return e, ratio


def set_switch(monkeypatch, c):
    if c["switch"]:
        monkeypatch.setenv(*c["switch"])


def slab_is_what_the_plan_wrote(name, slab, written):
    """slab [chunks, per]: the first `written` chunks hold finite values everywhere, the rest still the NaN poison."""
    assert bool(torch.isfinite(slab[:written]).all()), f"{name}: a slab element of the {written} chunks of the plan was never written"
    assert bool(torch.isnan(slab[written:]).all()), f"{name}: a slab chunk past the {written} of the plan was written"


def assert_signs_decided(x, sc, sh, grp):
    x = x.double()
    if grp:
        sc, sh = (t.repeat_interleave(grp, 0).view(x.shape[0], 1, 1, -1) for t in (sc, sh))
    assert G.undecided_signs(x, sc, sh, x * sc.double() + sh.double())[1] == 0


# ================================================================================================ single-layer launches
class Single:
    """One case on the device: launches sst_conv_wgrad_grp in a form and a mode, checks slab, guards and the untouched dW of a deferred
    reduce, -> dW on the device."""

    def __init__(self, ops, c, d):
        self.ops, self.c, self.d, self.L = ops, c, d, ops._abi.lib()
        self.x, self.dy, self.sc, self.sh, self.base = (dev(d[k]) for k in ("x", "dy", "sc", "sh", "base"))
        self.slopes = {s: torch.tensor([s], device="cuda") for s in (R.SLOPE, R.SELECT_SLOPE)}

    def launch(self, form, mode):
        ops, c, L = self.ops, self.c, self.L
        B, H, W, cin, cout, k, s = c["shape"]
        truth, from_dev = LAUNCH_FORMS[form]
        aff, slope = R.FORMS[truth]
        act = R.ACT_SLOPE if slope is not None else R.ACT_NONE
        bits = MODES[mode]
        p = R.case_plan(c, aff, act)
        per = k * k * cout * cin
        nch, pend = L.sst_conv_wgrad_chunks2(*c["shape"], 1), L.sst_conv_wgrad_pending_reduce(*c["shape"], int(aff), act)
        assert (nch, pend) == (p["slab_chunks"], p["pending"]) and p["name"] == c["name"]
        gd = G.Guarded()
        slab = gd.empty(nch, per, fill=NAN)
        dw = gd.put(self.d["base"]) if bits & 1 else gd.empty(cout, cin, k, k, fill=NAN)
        sl = self.slopes[slope] if from_dev else None
        rc = L.sst_conv_wgrad_grp(self.x.data_ptr(), self.dy.data_ptr(), slab.data_ptr(), dw.data_ptr(), self.sc.data_ptr() if aff else None,
                                  self.sh.data_ptr() if aff else None, sl.data_ptr() if from_dev else None,
                                  0.0 if from_dev or slope is None else slope, act, B, H, W, cin, cout, s, k, bits, c["grp"] if aff else 0,
                                  ops._abi.stream_ptr())
        ops._abi.check(rc, f"sst_conv_wgrad_grp {c['id']} {form} {mode}")
        tag = f"{c['id']} {form} {mode}"
        if bits & 4 and pend:
            untouched = torch.equal(dw, self.base) if bits & 1 else bool(torch.isnan(dw).all())
            assert untouched, f"{tag}: dW was written before the deferred reduce"
            ops.wgrad_reduce_flush([(slab, dw, pend, k * k, cout, cin, bits & 1)])
        written = p["nchunk"] if pend or p["kind"] == "k3c3_mfma" else 0
        slab_is_what_the_plan_wrote(tag, slab, written)
        gd.check()
        self.partials = slab[:written]
        return dw

    def slab_sum64(self):
        """The chunk partials of the last launch summed in fp64, in dW's layout: the slab against the truth, before any reduce."""
        _, _, _, cin, cout, k, _ = self.c["shape"]
        return self.partials.double().sum(0).view(k * k, cout, cin).permute(1, 2, 0).reshape(cout, cin, k, k).cpu()


def check_single(ops, monkeypatch, worst, c, integer):
    set_switch(monkeypatch, c)
    L = ops._abi.lib()
    B, H, W, cin, cout, k, s = c["shape"]
    assert L.sst_conv_wgrad_kernel_name(*c["shape"], 1).decode() == c["name"]
    d = R.single_data(c["id"], integer)
    P = R.chain_length(c)
    if not integer and c["affine"]:
        assert_signs_decided(d["x"], d["sc"], d["sh"], c["grp"])
    run = Single(ops, c, d)
    p = R.case_plan(c)
    print(f"\n[{c['id']}] {c['shape']} {c['name']}  chunks {p['nchunk']} of slab {p['slab_chunks']}, pending {p['pending']}, "
          f"P = {P}, {'integers' if integer else 'random'}")
    base64 = d["base"].double()
    got = {}
    for form, (truth, _) in LAUNCH_FORMS.items():
        if truth not in d["refs"]:
            continue
        ref, terms = d["refs"][truth]
        for mode, bits in MODES.items():
            dw = run.launch(form, mode)
            if mode == "write" and run.partials.shape[0]:          # the slab itself, chunk partials summed in fp64: right before any reduce
                if integer:
                    assert torch.equal(run.slab_sum64(), ref), f"{c['id']} {form}: the slab's chunk partials do not sum to the fp64 dW"
                else:
                    G.assert_elementwise(f"slab sum {c['id']} {form}", run.slab_sum64(), ref, terms, P + 8)
            assert torch.equal(dw, run.launch(form, mode)), f"{c['id']} {form} {mode}: second launch differs"
            acc = bits & 1
            e, ratio = held(f"dW {c['id']} {form} {mode}", dw, ref + base64 if acc else ref, terms + base64.abs() if acc else terms, P + 8, integer)
            got[form, mode] = dw
            if not integer:
                note(worst, c["name"], truth, ratio)
                print(f"  {form:18s} {mode:20s} norm-wise {e:.2e}   worst elementwise {ratio:7.2f}   (bound k = {P + 8})")
        assert torch.equal(got[form, "write"], got[form, "deferred"]), f"{c['id']} {form}: the deferred reduce differs from the launch's own"
        assert torch.equal(got[form, "accumulate"], got[form, "deferred accumulate"]), f"{c['id']} {form}: deferred accumulate differs"
    if c["affine"]:
        for mode in MODES:
            assert torch.equal(got["affine", mode], got["affine slope-dev", mode]), f"{c['id']} {mode}: the slope from the device changes dW"
    return got


@pytest.mark.parametrize("integer", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_single_layer_against_fp64(ops, monkeypatch, worst, c, integer):
    got = check_single(ops, monkeypatch, worst, c, integer)
    if c["id"] == "tap_1x1_maps":                          # 1 x 1 maps: only the centre tap ever meets a pixel
        for dw in got.values():
            centre = torch.zeros(3, 3, dtype=torch.bool)
            centre[1, 1] = True
            off = dw.cpu()[:, :, ~centre]
            want = R.single_data(c["id"], integer)["base"][:, :, ~centre]
            assert bool((off == 0).all()) or torch.equal(off, want), "a tap outside the 1 x 1 map is not exactly zero"


@pytest.mark.parametrize("cid, bad", [("tile_groups_goff_in_wave", 3), ("tile_groups_per_image", 2)])
def test_groups_that_do_not_divide_the_batch_are_refused(ops, monkeypatch, cid, bad):
    c = R.BY_ID[cid]
    set_switch(monkeypatch, c)
    L = ops._abi.lib()
    B, H, W, cin, cout, k, s = c["shape"]
    ho, wo = R.out_hw(H, W, k, s)
    assert B % bad and not L.sst_conv_wgrad_groups_ok(*c["shape"], bad) and L.sst_conv_wgrad_groups_ok(*c["shape"], c["grp"])
    gd = G.Guarded()
    x, dy, co = gd.empty(B, H, W, cin, fill=1.0), gd.empty(B, ho, wo, cout, fill=1.0), gd.empty(B, cin, fill=1.0)
    slab = gd.empty(L.sst_conv_wgrad_chunks2(*c["shape"], 1) * 9 * cout * cin, fill=NAN)
    dw = gd.empty(cout, cin, 3, 3, fill=NAN)
    rc = L.sst_conv_wgrad_grp(x.data_ptr(), dy.data_ptr(), slab.data_ptr(), dw.data_ptr(), co.data_ptr(), co.data_ptr(), None, R.SLOPE, R.ACT_SLOPE,
                              B, H, W, cin, cout, s, k, 0, bad, ops._abi.stream_ptr())
    assert rc != 0 and b"coefficient groups" in L.sst_last_error()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(slab).all())
    gd.check()


# ================================================================================================ the grouped entry
def job_table(rows):
    flat = [w for r in rows for w in r]
    return (ctypes.c_longlong * len(flat))(*flat)


class Grouped:
    """njobs layers of one shape through sst_conv_wgrad_grouped, each job with the coefficients of its form."""

    def __init__(self, ops, c, jobs):
        self.ops, self.c, self.jobs, self.L = ops, c, jobs, ops._abi.lib()
        self.dv = [{k: dev(j[k]) for k in ("x", "dy", "sc", "sh", "base")} for j in jobs]
        self.slope_dev = torch.tensor([R.SELECT_SLOPE], device="cuda")

    def job_args(self, i):
        """-> (in_scale, in_shift, in_slope, in_slope_const, in_act) of job i, tensors on the device."""
        sc, sh, slope, from_dev = R.job_form(self.jobs[i]["form"], self.dv[i]["sc"], self.dv[i]["sh"])
        return sc, sh, self.slope_dev if from_dev else None, 0.0 if from_dev or slope is None else slope, R.ACT_SLOPE if slope is not None else R.ACT_NONE

    def launch(self, accumulate, njobs=None, expect_refusal=False):
        ops, c, L = self.ops, self.c, self.L
        B, H, W, cin, cout, k, s = c["shape"]
        n = njobs or len(self.jobs)
        per = k * k * cout * cin
        nch = L.sst_conv_wgrad_chunks2(*c["shape"], n)
        gd = G.Guarded()
        slab = gd.empty(n, nch, per, fill=NAN)
        dws = [gd.put(self.jobs[i]["base"]) if accumulate else gd.empty(cout, cin, k, k, fill=NAN) for i in range(n)]
        rows = []
        for i in range(n):
            sc, sh, sl, slc, act = self.job_args(i)
            bits = struct.unpack("<q", struct.pack("<fi", slc, act))[0]
            rows.append([self.dv[i]["x"].data_ptr(), self.dv[i]["dy"].data_ptr(), slab[i].data_ptr(), dws[i].data_ptr(), sc.data_ptr() if sc is not None else 0,
                         sh.data_ptr() if sh is not None else 0, sl.data_ptr() if sl is not None else 0, bits])
        arr = job_table(rows)
        rc = L.sst_conv_wgrad_grouped(ctypes.cast(arr, ctypes.c_void_p), n, B, H, W, cin, cout, s, k, int(accumulate), ops._abi.stream_ptr())
        if expect_refusal:
            assert rc < 0 and str(R.WG_TAB_MAX).encode() in L.sst_last_error(), (rc, L.sst_last_error())
            assert bool(torch.isnan(slab).all()) and all(bool(torch.isnan(d).all()) for d in dws), "a refused call launched"
            gd.check()
            return None
        ops._abi.check(rc, f"sst_conv_wgrad_grouped {c['id']}")
        p = R.plan(*c["shape"], njobs=n, grouped=True, env=R.env_of(c))
        assert nch == p["slab_chunks"]
        for i in range(n):
            slab_is_what_the_plan_wrote(f"{c['id']} job {i}", slab[i], p["nchunk"])
        gd.check()
        return dws


@pytest.mark.parametrize("integer", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("c", R.GROUPED, ids=[c["id"] for c in R.GROUPED])
def test_grouped_entry_against_fp64(ops, monkeypatch, worst, c, integer):
    """Every job against the truth of its own coefficients, with accumulate = 0 and = 1."""
    set_switch(monkeypatch, c)
    L = ops._abi.lib()
    n = c["njobs"]
    assert L.sst_conv_wgrad_kernel_name(*c["shape"], n).decode() == c["name"]
    jobs = R.grouped_data(c["id"], integer)
    assert {j["form"] for j in jobs} == set(R.JOB_FORMS)
    P = R.chain_length(c)
    if not integer:
        for j in jobs:
            assert_signs_decided(j["x"], j["sc"], j["sh"], 0)
    run = Grouped(ops, c, jobs)
    p = R.case_plan(c)
    print(f"\n[{c['id']}] {n} jobs of {c['shape']} {c['name']}  chunks {p['nchunk']} of slab {p['slab_chunks']}, P = {P}, "
          f"{'integers' if integer else 'random'}")
    for accumulate in (0, 1):
        dws = run.launch(accumulate)
        again = run.launch(accumulate)
        errs, ratios = [], []
        for i, (j, dw) in enumerate(zip(jobs, dws)):
            assert torch.equal(dw, again[i]), f"{c['id']} job {i}: second launch differs"
            ref, terms = j["ref"]
            b = j["base"].double()
            e, r = held(f"dW {c['id']} job {i} ({j['form']}) accumulate {accumulate}", dw, ref + b if accumulate else ref,
                        terms + b.abs() if accumulate else terms, P + 8, integer)
            errs.append(e)
            ratios.append(r)
            if not integer:
                note(worst, c["name"] + " (grouped)", "plain" if j["form"] == "plain" else "affine", r)
        if not integer:
            print(f"  accumulate {accumulate}: norm-wise {max(errs):.2e}   worst elementwise {max(ratios):7.2f}   (bound k = {P + 8})")


def test_grouped_entry_refuses_41_jobs_and_wgrad_group_splits_them(ops, monkeypatch):
    """41 jobs: the entry refuses them with no launch and names the cap; ops.WgradGroup runs them as 40 + 1, all 41 exact."""
    c = R.BY_ID["grouped_band7_40_jobs"]
    set_switch(monkeypatch, c)
    B, H, W, cin, cout, k, s = c["shape"]
    n = R.WG_TAB_MAX + 1
    jobs = R.grouped_data(c["id"], True, n)
    run = Grouped(ops, c, jobs)
    run.launch(0, n, expect_refusal=True)
    gd = G.Guarded()
    dws = [gd.empty(cout, cin, k, k, fill=NAN) for _ in range(n)]
    grp = ops.WgradGroup()
    for i in range(n):
        sc, sh, sl, slc, act = run.job_args(i)
        grp.add(run.dv[i]["x"], run.dv[i]["dy"], dws[i], k, s, in_scale=sc, in_shift=sh, in_slope=sl, in_slope_const=slc, in_act=act)
    with gd.patch(ops):
        grp.run()
    for i, (j, dw) in enumerate(zip(jobs, dws)):
        same(f"dW job {i} of 41 ({j['form']})", dw, j["ref"][0])


# ================================================================================================ the slab reduces
REDUCE_JOBS = ["tap_wo70", "tap_wo100_full_block", "tile_s2_tw8", "tap_partial_blocks", "tap_scalar_s2_odd", "c3_valu_cout20"]
REDUCE_BIG = "tile_s1_tw6_big_dw"                      # once: the vector form's capped grid inside the multi-job launch


@pytest.mark.parametrize("integer", DATA, ids=DATA_IDS)
def test_reduce_multi_25_jobs(ops, monkeypatch, integer):
    """One wgrad_reduce_flush over 25 deferred jobs (24 + 1) mixing the split, vector and scalar forms and both accumulate flags: every
    dW against fp64 (bit-equal on integers) and bit-identical to the per-layer reduce of the same slab; 25 jobs passed straight to
    sst_wgrad_reduce_multi are refused."""
    monkeypatch.setenv(*R.S1T)                             # the route of REDUCE_BIG; no other job's shape is taken by the tile kernel at stride 1
    L = ops._abi.lib()
    ids = [REDUCE_JOBS[i % len(REDUCE_JOBS)] for i in range(R.WR_TAB_MAX)] + [REDUCE_BIG]
    ids[0], ids[-1] = ids[-1], ids[0]                      # the 25th job (a launch of its own) is a split one, the big one shares the 24
    assert len(ids) == R.WR_TAB_MAX + 1
    runs, variants = {}, set()
    for cid in set(ids):
        c = R.BY_ID[cid]
        p = R.plan(*c["shape"], env=dict([R.S1T]))
        assert p["name"] == c["name"] == L.sst_conv_wgrad_kernel_name(*c["shape"], 1).decode() and p["pending"] > 0
        variants.add(R.reduce_variant(p["pending"], c["shape"][3]))
        runs[cid] = (Single(ops, c, R.single_data(cid, integer)), p)
    assert variants == {"split", "vector", "scalar"} and R.reduce_blocks(2, 9, 512, 256)[1]
    assert R.reduce_variant(runs[ids[-1]][1]["pending"], R.BY_ID[ids[-1]]["shape"][3]) == "split"
    gd = G.Guarded()
    deferred, outs = [], []
    for i, cid in enumerate(ids):
        run, p = runs[cid]
        B, H, W, cin, cout, k, s = run.c["shape"]
        acc = i & 1 if i else 1                            # both flags among the 24 and the big job accumulates
        slab = gd.empty(p["slab_chunks"], k * k * cout * cin, fill=NAN)
        dw = gd.put(run.d["base"]) if acc else gd.empty(cout, cin, k, k, fill=NAN)
        ops._abi.check(L.sst_conv_wgrad_grp(run.x.data_ptr(), run.dy.data_ptr(), slab.data_ptr(), dw.data_ptr(), None, None, None, 0.0, R.ACT_NONE,
                                            B, H, W, cin, cout, s, k, acc | 4, 0, ops._abi.stream_ptr()), "sst_conv_wgrad_grp")
        deferred.append((slab, dw, p["pending"], k * k, cout, cin, acc))
        outs.append((cid, acc, dw))
    assert {a for _, a, _ in outs} == {0, 1}
    pack = lambda js: b"".join(struct.pack("<QQiiiiii", sl.data_ptr(), dw.data_ptr(), nch, kk, co, ci, a, 0) for sl, dw, nch, kk, co, ci, a in js)
    assert L.sst_wgrad_reduce_multi(ctypes.c_char_p(pack(deferred)), len(deferred), ops._abi.stream_ptr()) != 0
    assert str(R.WR_TAB_MAX).encode() in L.sst_last_error()
    torch.cuda.synchronize()
    for cid, acc, dw in outs:                              # the refused call launched nothing
        assert torch.equal(dw, runs[cid][0].base) if acc else bool(torch.isnan(dw).all())
    jobs = list(deferred)
    ops.wgrad_reduce_flush(jobs)
    assert not jobs
    gd.check()
    for i, (cid, acc, dw) in enumerate(outs):
        run, p = runs[cid]
        ref, terms = run.d["refs"]["plain"]
        b = run.d["base"].double()
        held(f"dW job {i} {cid} accumulate {acc}", dw, ref + b if acc else ref, terms + b.abs() if acc else terms, R.chain_length(run.c) + 8, integer)
        assert torch.equal(dw, run.launch("plain", "accumulate" if acc else "write")), f"job {i} {cid}: differs from the per-layer reduce"
