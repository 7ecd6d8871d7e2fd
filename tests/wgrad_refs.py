"""The weight gradient of the NHWC convolution in plain torch fp64, the launch plans of csrc/conv_wgrad.hip restated in Python, and the
one list of cases tests/test_conv_wgrad_fp64_gpu.py runs.  No GPU, no library: tests/test_wgrad_refs.py holds `wgrad64` to fp64
autograd, the restated plans to the built library's host entries, and every case to the branch it was chosen for.

Tensors are NHWC: x [B, H, W, Cin], dy [B, Ho, Wo, Cout]; dW is the reference layout [Cout, Cin, k, k]."""
import functools

import torch
import torch.nn.functional as F

SUB, CONV_NT, WLD = 64, 256, 68                  # conv_wgrad.hip: pixels per staged sub-tile, threads per workgroup, LDS row stride
WB_XS, WB_DS, C3_ROWS, C3M_TPW = 10, 3, 8, 4
WG_TAB_MAX, WR_TAB_MAX = 40, 24                  # jobs per grouped launch / per multi-reduce launch
ACT_NONE, ACT_SLOPE = 0, 1


# ================================================================================================ the truth
def out_hw(H, W, k, s):
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def act_input(x, scale=None, shift=None, slope=None, grp=0):
    """x' = act(x * scale + shift) in fp64: scale / shift [Cin], or [B / grp, Cin] with image b on row b // grp; slope None = no
    activation."""
    x = x.double()
    B, cin = x.shape[0], x.shape[-1]
    if scale is not None:
        rows = lambda c: c.double().view(-1, cin).repeat_interleave(grp if grp else B, 0).view(B, 1, 1, cin)
        x = x * rows(scale) + rows(shift)
    if slope is not None:
        x = torch.where(x > 0, x, x * float(slope))
    return x


def wgrad64(x, dy, k, stride, scale=None, shift=None, slope=None, grp=0):
    """-> (dW64, terms64): dW[co, ci, ky, kx] = sum_{b, oy, ox} x'[b, oy s + ky - p, ox s + kx - p, ci] dy[b, oy, ox, co] with x' zero
    outside the image (padded AFTER the activation), one shifted einsum per tap; terms64 is the same sum over magnitudes."""
    xa, dy = act_input(x, scale, shift, slope, grp), dy.double()
    p = k // 2
    Ho, Wo = out_hw(x.shape[1], x.shape[2], k, stride)
    assert tuple(dy.shape[:3]) == (x.shape[0], Ho, Wo), (tuple(x.shape), tuple(dy.shape), k, stride)
    xp = F.pad(xa, (0, 0, p, p, p, p))
    xm, dm = xp.abs(), dy.abs()
    dw = torch.zeros(dy.shape[-1], x.shape[-1], k, k, dtype=torch.float64)
    terms = torch.zeros_like(dw)
    for ky in range(k):
        for kx in range(k):
            win = (slice(None), slice(ky, ky + (Ho - 1) * stride + 1, stride), slice(kx, kx + (Wo - 1) * stride + 1, stride))
            dw[:, :, ky, kx] = torch.einsum("bhwi,bhwo->oi", xp[win], dy)
            terms[:, :, ky, kx] = torch.einsum("bhwi,bhwo->oi", xm[win], dm)
    return dw, terms


def exact(bound, unit):
    """`bound`: the largest sum of magnitudes a chain can reach, all of whose terms are multiples of `unit` (a power of two): below
    2^24 unit every fp32 partial sum is exact whatever the order."""
    assert float(bound) / unit < 2 ** 24, f"sums up to {float(bound)} in units of {unit} leave the exact range of fp32"


# ================================================================================================ the plans, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def _env(env, name):
    return (env or {}).get(name)


def tile_plan(B, H, W, Cin, Cout, k, s, env=None):
    """wgrad_s2_plan -> None or dict(th, tw, ntiles, tpc, nchunk, tiles_x, tiles_y, last) (last: tiles of the last chunk)."""
    if k != 3 or s not in (1, 2) or Cin % 32 or Cout % 32 or B <= 0:
        return None
    if s == 2 and (H | W) & 1:
        return None
    force = False
    e = _env(env, "SST_WGRAD_S2" if s == 2 else "SST_WGRAD_S1T")
    if e is not None:
        if int(e) == 0:
            return None
        force = True
    Ho, Wo = H // s, W // s
    th = tw = 0
    if s == 2:
        if Wo % 8 == 0 and Ho % 2 == 0:
            th, tw = 2, 8
        elif Wo % 6 == 0 and Ho % 2 == 0:
            th, tw = 2, 6
    else:
        if 2.0 * B * H * W * Cin * Cout * 9 < 2.5e9 and not force:
            return None
        if Wo % 8 == 0 and Ho % 4 == 0:
            th, tw = 4, 8
        elif Wo % 6 == 0 and Ho % 4 == 0:
            th, tw = 4, 6
    if not th or B * H * W * Cin >= 2 ** 31:
        return None
    ntiles = B * (Ho // th) * (Wo // tw)
    nblk = (Cout // 32) * (Cin // 32)
    nchunk = max(256 // nblk, 1)
    tpc = max(_cdiv(_cdiv(ntiles, nchunk), 8) * 8, 8)
    nchunk = _cdiv(ntiles, tpc)
    return dict(th=th, tw=tw, ntiles=ntiles, tpc=tpc, nchunk=nchunk, tiles_x=Wo // tw, tiles_y=Ho // th, last=ntiles - (nchunk - 1) * tpc)


def band_plan(B, H, W, Cin, Cout, k, s, njobs=1, env=None):
    """wgrad_band_plan -> None or dict(R, bpc, nchunk, nbands, xslots, lds, last) (last: bands of the last chunk)."""
    if k != 3 or s != 1 or Cin % 64 or Cout % 64 or W % 4 or W < 4:
        return None
    e = _env(env, "SST_WGRAD_BAND")
    if e is not None and int(e) == 0:
        return None
    if 2.0 * B * H * W * Cin * Cout * 9 * njobs < 2.5e9 and e is None:
        return None
    nblk = (Cout // 64) * (Cin // 64)
    slots = int(_env(env, "SST_WGRAD_BAND_SLOTS") or 512)
    rmax = int(_env(env, "SST_WGRAD_BAND_R") or 2)
    best, best_cost = None, 1e30
    for R in range(rmax, 0, -1):
        if H % R:
            continue
        npx_x, npx_d = (R + 2) * (W + 2), R * W
        xslots = _cdiv(npx_x * 16, CONV_NT)
        if xslots > WB_XS or _cdiv(npx_d * 16, CONV_NT) > WB_DS:
            continue
        lds = (npx_x + npx_d) * WLD * 4
        if lds > 78 * 1024:
            continue
        nbands, per = B * (H // R), nblk * njobs
        bpc = max(_cdiv(nbands * per, slots), 1)
        nchunk = _cdiv(nbands, bpc)
        rounds = _cdiv(nchunk * per, slots)
        cost = float(rounds) * (float(bpc) * R + 1.4)
        if cost < best_cost:
            best_cost = cost
            best = dict(R=R, bpc=bpc, nchunk=nchunk, nbands=nbands, xslots=xslots, lds=lds, last=nbands - (nchunk - 1) * bpc)
    return best


def _general_chunks(M, Cin, Cout, k):
    nblk = _cdiv(Cout, 64) * _cdiv(Cin, 64)
    want = max(min(_cdiv(1024, k * k * nblk), _cdiv(M, 160)), 1)
    chunk_px = _cdiv(_cdiv(M, want), SUB) * SUB
    return _cdiv(M, chunk_px)


def general_plan(B, H, W, Cin, Cout, k, s, njobs=1, grouped=False, env=None):
    """sst_conv_wgrad_chunks with the grouped re-chunking of wgrad_plan -> dict(nchunk, slab_chunks, chunk_px, M, last_px)
    (slab_chunks without the 3-channel kernels' share: see plan())."""
    Ho, Wo = out_hw(H, W, k, s)
    M = B * Ho * Wo
    nchunk = slab_chunks = _general_chunks(M, Cin, Cout, k)
    if grouped:
        target = int(_env(env, "SST_WGRAD_GROUP_WGS") or 2048)
        nblk = _cdiv(Cout, 64) * _cdiv(Cin, 64)
        want = max(_cdiv(target, k * k * nblk * njobs), 1)
        if target > 0 and want < nchunk:
            nchunk = _cdiv(M, _cdiv(_cdiv(M, want), SUB) * SUB)
    chunk_px = _cdiv(_cdiv(M, nchunk), SUB) * SUB
    return dict(nchunk=nchunk, slab_chunks=slab_chunks, chunk_px=chunk_px, M=M, last_px=M - (nchunk - 1) * chunk_px)


def k3c3_chunks(B, H, W):
    """k3c3_mfma_chunks: 32-pixel row segments, 4 waves x C3M_TPW segments per workgroup."""
    return _cdiv(B * H * (W >> 5), 4 * C3M_TPW)


def plan(B, H, W, Cin, Cout, k, s, njobs=1, has_scale=False, act=ACT_NONE, grouped=None, env=None):
    """wgrad_plan -> dict(kind, name, nchunk, pending, slab_chunks, sub) with sub the tile / band / general plan of the kind.
    grouped None: as the sizing and naming entries take it (njobs > 1)."""
    grouped = njobs > 1 if grouped is None else grouped
    t = None if grouped else tile_plan(B, H, W, Cin, Cout, k, s, env)
    if t:
        direct = t["nchunk"] == 1 and _env(env, "SST_WGRAD_TILE_NO_DIRECT") is None
        return dict(kind="tile", name=f"conv_wgrad_tile_kernel<{s}, {t['th']}, {t['tw']}, 8>", nchunk=t["nchunk"], slab_chunks=t["nchunk"],
                    pending=0 if direct else t["nchunk"], sub=t)
    b = band_plan(B, H, W, Cin, Cout, k, s, njobs, env)
    if b:
        return dict(kind="band", name=f"conv_wgrad_band_kernel<{7 if b['xslots'] <= 7 else 10}>", nchunk=b["nchunk"], slab_chunks=b["nchunk"],
                    pending=0 if grouped else b["nchunk"], sub=b)
    g = general_plan(B, H, W, Cin, Cout, k, s, njobs, grouped, env)
    slab_chunks = g["slab_chunks"]
    if Cin == 3 and k == 3 and s == 1:
        rows = B * _cdiv(H, C3_ROWS)
        mfma = W % 32 == 0 and Cout == 64 and _env(env, "SST_WGRAD_NO_K3C3_MFMA") is None
        slab_chunks = max(slab_chunks, rows, k3c3_chunks(B, H, W) if mfma else 0)
        if not grouped and not has_scale and act == ACT_NONE:
            if mfma:
                return dict(kind="k3c3_mfma", name="wgrad_k3c3_mfma_kernel", nchunk=k3c3_chunks(B, H, W), slab_chunks=slab_chunks, pending=0,
                            sub=dict(segments=B * H * (W >> 5)))
            if _env(env, "SST_WGRAD_NO_K3C3") is None:
                return dict(kind="k3c3", name="wgrad_k3c3_kernel", nchunk=rows, slab_chunks=slab_chunks, pending=rows,
                            sub=dict(rows_last=H - (_cdiv(H, C3_ROWS) - 1) * C3_ROWS))
    vec = Cin % 4 == 0 and Cout % 4 == 0
    return dict(kind="general", name=f"conv_wgrad_kernel<{'true' if vec else 'false'}>", nchunk=g["nchunk"], slab_chunks=slab_chunks,
                pending=0 if grouped else g["nchunk"], sub=g)


def groups_ok(B, H, W, Cin, Cout, k, s, grp, env=None):
    """sst_conv_wgrad_groups_ok."""
    return int(grp > 0 and B > 0 and B % grp == 0 and plan(B, H, W, Cin, Cout, k, s, 1, True, ACT_NONE, False, env)["kind"] == "tile")


def reduce_variant(nchunk, Cin):
    """launch_wgrad_reduce / wgrad_reduce_multi_kernel: which of the three forms sums a slab."""
    return "split" if Cin % 4 == 0 and nchunk >= 8 else "vector" if Cin % 4 == 0 else "scalar"


def reduce_blocks(nchunk, KK, Cout, Cin):
    """Workgroups of the slab reduce and whether its grid is capped (the vector / scalar forms then walk a stride loop)."""
    total = KK * Cout * Cin
    if reduce_variant(nchunk, Cin) == "split":
        return _cdiv(total // 4, 64), False
    items = total // 4 if Cin % 4 == 0 else total
    return min(_cdiv(items, 256), 1024), _cdiv(items, 256) > 1024


# ================================================================================================ the cases
def case(id, shape, name, switch=None, grp=0, njobs=1, affine=True, expect=None, props=None, why=""):
    """shape (B, H, W, Cin, Cout, k, s); switch: the environment switch the route needs; name: the kernel the library must name;
    expect: plan numbers that must come out exactly; props: predicate on plan() for the branch the case was chosen for."""
    return dict(id=id, shape=shape, name=name, switch=switch, grp=grp, njobs=njobs, affine=affine, expect=expect or {},
                props=props or (lambda p: True), why=why)


S1T, BAND = ("SST_WGRAD_S1T", "1"), ("SST_WGRAD_BAND", "1")
_tile = "conv_wgrad_tile_kernel<%d, %d, %d, 8>"

CASES = [
    # ---- all-taps tile kernel
    case("tile_s2_tw8", (3, 12, 32, 64, 96, 3, 2), _tile % (2, 2, 8), expect=dict(ntiles=18, tpc=8, nchunk=3, last=2),
         props=lambda p: p["pending"] == 3 and p["sub"]["tiles_x"] == 2 and p["sub"]["tiles_y"] == 3,
         why="six idle waves in the last chunk, interior and top / left edge tiles, two input-channel blocks"),
    case("tile_s2_tw6_direct", (2, 8, 24, 32, 32, 3, 2), _tile % (2, 2, 6), expect=dict(ntiles=8, nchunk=1),
         props=lambda p: p["pending"] == 0, why="direct dW store and in-kernel accumulate, no slab"),
    case("tile_s1_tw8", (3, 12, 24, 32, 32, 3, 1), _tile % (1, 4, 8), S1T, expect=dict(ntiles=27, nchunk=4, last=3),
         props=lambda p: p["sub"]["tiles_x"] == 3 and p["sub"]["tiles_y"] == 3, why="3 x 3 tiles per image: one interior tile, all eight edge kinds"),
    case("tile_s1_tw6_one_tile", (3, 4, 6, 32, 64, 3, 1), _tile % (1, 4, 6), S1T, expect=dict(ntiles=3, nchunk=1),
         props=lambda p: p["sub"]["tiles_x"] == 1 and p["sub"]["tiles_y"] == 1 and p["pending"] == 0,
         why="tiles_x == tiles_y == 1: every patch border masked at once"),
    case("tile_s1_tw6_big_dw", (2, 12, 12, 256, 512, 3, 1), _tile % (1, 4, 6), S1T, expect=dict(ntiles=12, nchunk=2, last=4),
         props=lambda p: reduce_variant(2, 256) == "vector" and reduce_blocks(2, 9, 512, 256) == (1024, True),
         why="1.18 M-float dW: the vector reduce's capped grid and stride loop"),
    case("tile_groups_goff_in_wave", (16, 4, 16, 512, 512, 3, 2), _tile % (2, 2, 8), grp=4, expect=dict(ntiles=16, tpc=16, nchunk=1),
         props=lambda p: p["sub"]["tiles_y"] * p["sub"]["tiles_x"] == 1 and all((w // 4) != ((w + 8) // 4) for w in range(8)),
         why="wave w takes tiles w and w + 8, in groups w / 4 and 2 + w / 4: goff changes between a wave's tiles"),
    case("tile_groups_per_image", (5, 8, 32, 32, 32, 3, 2), _tile % (2, 2, 8), grp=1, expect=dict(ntiles=20, nchunk=3),
         props=lambda p: p["sub"]["tiles_y"] * p["sub"]["tiles_x"] == 4, why="one group per image: five distinct coefficient rows"),
    # ---- band kernel
    case("band7_R2", (22, 12, 24, 64, 128, 3, 1), "conv_wgrad_band_kernel<7>", BAND, expect=dict(R=2, nbands=132, bpc=1, xslots=7),
         props=lambda p: (2 + 2) * (24 + 2) * 16 % CONV_NT != 0, why="R = 2 in a single-layer launch, 7 patch slots with the last partial, top and bottom masks"),
    case("band7_nblk6", (2, 5, 32, 128, 192, 3, 1), "conv_wgrad_band_kernel<7>", BAND, expect=dict(R=1, nbands=10, xslots=7),
         props=lambda p: (192 // 64, 128 // 64) == (3, 2), why="nblk = 6, asymmetric: a cob / cib swap shows"),
    case("band10", (2, 3, 48, 128, 64, 3, 1), "conv_wgrad_band_kernel<10>", BAND, expect=dict(R=1, nbands=6, xslots=10),
         props=lambda p: _cdiv(48 * 16, CONV_NT) == 3, why="every X slot and all 3 dY slots of the wide instance"),
    case("band10_two_blocks_each_side", (2, 3, 48, 128, 128, 3, 1), "conv_wgrad_band_kernel<10>", BAND, expect=dict(R=1, nbands=6, xslots=10),
         props=lambda p: (128 // 64, 128 // 64) == (2, 2), why="the 10-slot patch with two channel blocks on each side"),
    case("band7_bpc2_partial", (5, 7, 8, 256, 256, 3, 1), "conv_wgrad_band_kernel<7>", BAND, expect=dict(R=1, nbands=35, bpc=2, nchunk=18, last=1),
         props=lambda p: 7 % 2 == 1 and reduce_variant(18, 256) == "split",
         why="bpc > 1 in a single layer, partial last chunk, chunks straddling images (7 bands per image), split reduce"),
    # ---- per-tap kernel
    case("tap_wo70", (3, 7, 70, 8, 12, 3, 1), "conv_wgrad_kernel<true>", expect=dict(M=1470, nchunk=8, chunk_px=192, last_px=126),
         props=lambda p: 192 % 70 != 0 and 126 % SUB != 0 and reduce_variant(8, 8) == "split",
         why="Wo > 64 (adv_y == 0), chunk edges mid-row, partial last sub-tile of a partial last chunk, split reduce"),
    case("tap_wo100_full_block", (3, 5, 100, 64, 64, 3, 1), "conv_wgrad_kernel<true>", expect=dict(nchunk=8, last_px=156),
         why="a full 64 x 64 block at Wo > 64, below the band threshold"),
    case("tap_1x1_maps", (70, 1, 1, 8, 8, 3, 1), "conv_wgrad_kernel<true>", expect=dict(nchunk=1, chunk_px=128, M=70),
         why="1 x 1 maps: the oy / Ho carry; eight taps must be exactly 0"),
    case("tap_partial_blocks", (1, 6, 10, 68, 132, 3, 1), "conv_wgrad_kernel<true>", expect=dict(nchunk=1),
         props=lambda p: 68 % 64 == 4 and 132 % 64 == 4, why="partial second channel block on both sides"),
    case("tap_scalar_s2_odd", (2, 9, 13, 6, 10, 3, 2), "conv_wgrad_kernel<false>", expect=dict(M=2 * 5 * 7),
         why="stride 2 on odd sizes, both tails scalar"),
    case("tap_scalar_x", (2, 5, 7, 6, 8, 3, 1), "conv_wgrad_kernel<false>", why="x side scalar, dy side vector"),
    case("tap_scalar_dy", (2, 5, 7, 8, 6, 3, 1), "conv_wgrad_kernel<false>", why="dy side scalar, x side vector"),
    case("tap_k9", (1, 12, 10, 4, 8, 9, 1), "conv_wgrad_kernel<true>", why="9 x 9: 81 taps"),
    case("tap_k1", (2, 7, 9, 8, 8, 1, 1), "conv_wgrad_kernel<true>", why="a size the entry accepts"),
    case("tap_k5", (2, 7, 9, 8, 8, 5, 1), "conv_wgrad_kernel<true>", why="a size the entry accepts"),
    case("tap_k7_s2", (2, 7, 9, 8, 8, 7, 2), "conv_wgrad_kernel<true>", why="a size the entry accepts"),
    # ---- 3-channel kernels (plain only: an input affine sends the shape to the per-tap kernel)
    case("c3_mfma_450_chunks", (75, 96, 32, 3, 64, 3, 1), "wgrad_k3c3_mfma_kernel", affine=False, expect=dict(segments=7200, nchunk=450),
         props=lambda p: p["nchunk"] > 7 * 64 and p["nchunk"] - 2 < 8 * 64,
         why="nchunk > 448: the reduce's unrolled loop for groups 0 and 1, then its tail"),
    case("c3_mfma_dead_waves", (3, 5, 64, 3, 64, 3, 1), "wgrad_k3c3_mfma_kernel", affine=False, expect=dict(segments=30, nchunk=2),
         props=lambda p: 30 % 16 != 0, why="dead waves (live == false), all four borders"),
    case("c3_valu_cout20", (2, 13, 9, 3, 20, 3, 1), "wgrad_k3c3_kernel", affine=False, expect=dict(nchunk=4, rows_last=5),
         why="co < Cout guard, 5-row last band, scalar reduce"),
    case("c3_valu_cout64", (2, 13, 9, 3, 64, 3, 1), "wgrad_k3c3_kernel", affine=False, expect=dict(nchunk=4, rows_last=5), why="one full channel block"),
    case("c3_valu_cout128", (2, 13, 9, 3, 128, 3, 1), "wgrad_k3c3_kernel", affine=False, expect=dict(nchunk=4, rows_last=5), why="the cob loop"),
]

# grouped launches (sst_conv_wgrad_grouped): njobs layers of one shape
GROUPED = [
    case("grouped_band7_40_jobs", (3, 5, 8, 64, 64, 3, 1), "conv_wgrad_band_kernel<7>", BAND, njobs=40,
         expect=dict(R=1, nbands=15, bpc=2, nchunk=8, last=1), props=lambda p: 5 % 2 == 1 and p["pending"] == 0,
         why="the full job table; a chunk spanning images 0 / 1"),
    case("grouped_tap_rechunk", (2, 24, 24, 4, 8, 9, 1), "conv_wgrad_kernel<true>", njobs=13, expect=dict(nchunk=2, chunk_px=576, slab_chunks=6),
         props=lambda p: p["slab_chunks"] == 6, why="re-chunking; the unused slab chunks stay NaN and are not read"),
    case("grouped_tap_job_coefficients", (2, 13, 9, 8, 8, 3, 1), "conv_wgrad_kernel<true>", njobs=5, expect=dict(nchunk=2, last_px=106),
         why="each job has its own coefficients: affine + slope, affine only, slope const only, slope from device, plain"),
]
JOB_FORMS = ["affine_slope", "affine", "slope_const", "slope_dev", "plain"]          # cycled over the jobs of a grouped case

BY_ID = {c["id"]: c for c in CASES + GROUPED}
assert len(BY_ID) == len(CASES) + len(GROUPED)


def env_of(c):
    return dict([c["switch"]]) if c["switch"] else {}


def case_plan(c, has_scale=False, act=ACT_NONE):
    return plan(*c["shape"], njobs=c["njobs"], has_scale=has_scale, act=act, grouped=c["njobs"] > 1, env=env_of(c))


def chain_length(c):
    """P = B Ho Wo: the products in one element's chain."""
    B, H, W, _, _, k, s = c["shape"]
    ho, wo = out_hw(H, W, k, s)
    return B * ho * wo


# ================================================================================================ the data of a case
SLOPE, SELECT_SLOPE = 0.25, -1.5               # LeakyReLU as max(v, slope v) / as a select (slope outside [0, 1])
FORMS = {"plain": (False, None), "affine": (True, SLOPE), "select": (True, SELECT_SLOPE)}      # form -> (input affine, slope)


def _draws(seed, integer):
    gen = torch.Generator().manual_seed(seed + (0 if integer else 7))
    if integer:
        val = lambda *s: torch.randint(-3, 4, s, generator=gen).float()
        scale = lambda *s: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, s, generator=gen)]
        shift = lambda *s: torch.randint(1, 4, s, generator=gen).float() * (2 * torch.randint(0, 2, s, generator=gen).float() - 1)
    else:
        val = lambda *s: torch.randn(*s, generator=gen)
        scale = lambda *s: torch.rand(*s, generator=gen) + 0.5
        shift = lambda *s: torch.randn(*s, generator=gen) * 0.3 + 0.5
    return val, scale, shift


def _seed(c):
    return sum((i + 1) * 131 * v for i, v in enumerate(c["shape"])) + 17 * c["grp"] + c["njobs"]


def group_rows(rows, cin, integer, scale, shift):
    """Coefficient rows [rows, Cin] that differ from each other in every channel."""
    if not integer:
        return scale(rows, cin), shift(rows, cin)
    assert rows <= 6
    c, g = torch.arange(cin).view(1, -1), torch.arange(rows).view(-1, 1)
    sc = torch.tensor([0.5, 1.0, 2.0])[(c + g) % 3]
    sh = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])[(c + 5 * g) % 6]
    return sc.contiguous(), sh.contiguous()


@functools.lru_cache(maxsize=2)
def single_data(cid, integer):
    """fp32-valued inputs of a single-layer case and, per form, (dW64, terms64): dict(x, dy, base, sc, sh, refs)."""
    c = BY_ID[cid]
    B, H, W, cin, cout, k, s = c["shape"]
    ho, wo = out_hw(H, W, k, s)
    val, scale, shift = _draws(_seed(c), integer)
    d = dict(x=val(B, H, W, cin), dy=val(B, ho, wo, cout), base=val(cout, cin, k, k))
    rows = B // c["grp"] if c["grp"] else 1
    sc, sh = group_rows(rows, cin, integer, scale, shift) if c["grp"] else (scale(cin), shift(cin))
    d["sc"], d["sh"] = sc, sh
    d["refs"] = {}
    for form, (aff, slope) in FORMS.items():
        if aff and not c["affine"]:
            continue
        d["refs"][form] = wgrad64(d["x"], d["dy"], k, s, sc if aff else None, sh if aff else None, slope, c["grp"] if aff else 0)
    if integer:
        for form, (dw, terms) in d["refs"].items():
            exact(terms.max() + 3, 1.0 if form == "plain" else 0.125)
    return d


def job_form(form, sc, sh):
    """-> (scale, shift, slope for the truth, slope from the device?) of a grouped job."""
    return {"affine_slope": (sc, sh, SLOPE, False), "affine": (sc, sh, None, False), "slope_const": (None, None, SLOPE, False),
            "slope_dev": (None, None, SELECT_SLOPE, True), "plain": (None, None, None, False)}[form]


@functools.lru_cache(maxsize=2)
def grouped_data(cid, integer, njobs=None):
    """Per job of a grouped case: dict(x, dy, base, sc, sh, form, ref = (dW64, terms64)); job j takes form JOB_FORMS[j % 5]."""
    c = BY_ID[cid]
    B, H, W, cin, cout, k, s = c["shape"]
    ho, wo = out_hw(H, W, k, s)
    val, scale, shift = _draws(_seed(c), integer)
    jobs = []
    for j in range(njobs or c["njobs"]):
        d = dict(x=val(B, H, W, cin), dy=val(B, ho, wo, cout), base=val(cout, cin, k, k), sc=scale(cin), sh=shift(cin), form=JOB_FORMS[j % len(JOB_FORMS)])
        sc, sh, slope, _ = job_form(d["form"], d["sc"], d["sh"])
        d["ref"] = wgrad64(d["x"], d["dy"], k, s, sc, sh, slope)
        if integer:
            exact(d["ref"][1].max() + 3, 0.125)
        jobs.append(d)
    return jobs
