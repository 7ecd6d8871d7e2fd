"""What the degradation tests (test_degrade_refs.py, test_degrade_gpu.py) share: an fp64 restatement of the stage
lr = quantise(clamp(bicubic_down(gt (*) k) + n)) that starts from the deg rows' fp32 values, the quantised
rule, and a fixed small arena.  A plain helper module; numpy only, apart from the tap tables of srganst.bicubic._contribute."""
import numpy as np

BOUND = 3e-5        # (K^2 + Ty + Tx + 4) * 2^-24 * sum|w| * max|x| for K = 21, Ty = Tx = 16, sum|w| = max|x| = 1: 2.84e-5

# ---- the fixed small arena: three uint8 random images (H, W), one of which a 24-px window fits exactly; and, for the one case
# with a 32-px crop, which none of the three holds, a fourth
ARENA_SIZES = [(37, 29), (24, 24), (41, 26)]
ARENA_SIZES_32 = ARENA_SIZES + [(45, 38)]


def arena_images(S):
    rng = np.random.default_rng(20211021)
    sizes = ARENA_SIZES_32 if S > 24 else ARENA_SIZES
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def arena_descriptors(images, S, B=8):
    """B descriptors (image, y0, x0, t), t = k % 8, over the windows of every image that holds an S x S one: the four corners,
    odd x0 (odd byte offsets: a pixel is 3 bytes) and, where the image is exactly S x S, the one window."""
    wins = []
    for n, im in enumerate(images):
        h, w = im.shape[:2]
        if h < S or w < S:
            continue
        for y0, x0 in ((0, 0), (h - S, w - S), (0, w - S), (h - S, 0), ((h - S) // 2, min(w - S, 1)), (min(h - S, 1), (w - S) // 2)):
            if (n, y0, x0) not in wins:
                wins.append((n, y0, x0))
    assert wins
    return [(*wins[(3 * k) % len(wins)], k % 8) for k in range(B)]


# ---- Philox4x32-10 in integer arithmetic
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key, rounds=10):
    """counter: four uint32 arrays (or ints), key: two -> four uint64 arrays holding the 32-bit outputs."""
    c = [np.asarray(v, np.uint64) & 0xFFFFFFFF for v in counter]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(rounds):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)             # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def gauss(n, k0, k1):
    """The n standard normals of one sample's LR elements e = 0..n-1, in fp64."""
    x = philox4x32([np.arange(n), 0, 0, 0], (k0, k1))
    u1 = ((x[0] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((x[1] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def unpack(row):
    """One deg row -> (qa, qb, qc, sigma_n as the fp32 values the kernel reads, in fp64; k0, k1)."""
    row = np.asarray(row, np.int32)
    q = row[:4].view(np.float32).astype(np.float64)
    k = row[4:6].view(np.uint32)
    return q[0], q[1], q[2], q[3], int(k[0]), int(k[1])


def weights(qa, qb, qc, K):
    """The normalised K x K weights [dy][dx] in fp64."""
    p = K // 2
    d = np.arange(-p, p + 1, dtype=np.float64)
    dy, dx = d[:, None], d[None, :]
    w = np.exp(-(qa * dx * dx + qb * dx * dy + qc * dy * dy))
    return w / w.sum()


def bicubic_matrices(H, W, scale):
    """The two passes of srganst.bicubic as dense fp64 matrices [oh, H], [ow, W] from _contribute's tables."""
    from srganst.bicubic import _contribute
    out = []
    for n in (H, W):
        w, idx = _contribute(n, int(n * (1.0 / scale)), 1.0 / scale)
        M = np.zeros((w.shape[0], n))
        np.add.at(M, (np.arange(w.shape[0])[:, None], idx.numpy()), w.double().numpy())
        out.append(M)
    return out


def degrade_reference(gt, deg, scale, ksize, quantise=True):
    """gt [B,3,H,W] (numpy or torch, the fp32 values), deg int32 [B,8] -> lr fp64 [B,3,H//scale,W//scale]."""
    gt = np.asarray(gt, np.float64)
    deg = np.asarray(deg, np.int32).reshape(-1, 8)
    B, C, H, W = gt.shape
    p = ksize // 2
    My, Mx = bicubic_matrices(H, W, scale)
    out = np.empty((B, C, My.shape[0], Mx.shape[0]))
    for b in range(B):
        qa, qb, qc, sn, k0, k1 = unpack(deg[b])
        x = gt[b]
        if not qa < 0:
            k = weights(qa, qb, qc, ksize)
            xp = np.pad(x, ((0, 0), (p, p), (p, p)), mode="reflect")
            win = np.lib.stride_tricks.sliding_window_view(xp, (ksize, ksize), axis=(1, 2))      # [C, H, W, K, K]
            x = np.einsum("chwij,ij->chw", win, k)
        v = np.einsum("oh,chw,pw->cop", My, x, Mx)
        if sn != 0:
            v = v + sn * gauss(v.size, k0, k1).reshape(v.shape)
        if quantise:
            if not (qa < 0 and sn == 0):
                v = np.clip(v, 0.0, 1.0)
            v = np.rint(255.0 * v) / 255.0
        out[b] = v
    return out


def is_degraded(deg):
    deg = np.asarray(deg, np.int32).reshape(-1, 8)
    q = deg[:, :4].copy().view(np.float32)
    return ~((q[:, 0] < 0) & (q[:, 3] == 0))


def quantised_range(ref_unq, deg, bound=BOUND):
    """The grid values (in 0..255 units) a kernel within `bound` of the unquantised fp64 reference may produce: per element the
    pair (lo, hi) = the reference moved by -bound / +bound, clamped where the sample is degraded, rounded.  lo == hi except where
    255 v lies within 255 * bound of a half-integer."""
    d = is_degraded(deg)[:, None, None, None]
    lo, hi = ref_unq - bound, ref_unq + bound
    lo, hi = np.where(d, np.clip(lo, 0, 1), lo), np.where(d, np.clip(hi, 0, 1), hi)
    return np.rint(255.0 * lo), np.rint(255.0 * hi)


def check_quantised(lr, ref_unq, deg, what=""):
    """lr (the kernel's quantised output, fp32) against the rule of the issue: every pixel equals rint(255 ref) / 255 or, where
    the reference alone says the rounding is ambiguous, differs from it by exactly one grid step.  Prints and returns the number
    of pixels that differ from the reference's own rounding."""
    lr = np.asarray(lr, np.float64)
    lo, hi = quantised_range(ref_unq, deg)
    assert (hi - lo).max() <= 1.0
    q = 255.0 * lr
    on_grid = np.abs(q - np.rint(q)) < 1e-3
    inside = (np.rint(q) >= lo) & (np.rint(q) <= hi)
    d = is_degraded(deg)[:, None, None, None]
    want = np.rint(255.0 * np.where(d, np.clip(ref_unq, 0, 1), ref_unq))
    differ = int((np.rint(q) != want).sum())
    print(f"{what}: {differ} of {lr.size} quantised pixels differ from the fp64 reference's rounding; {int((lo != hi).sum())} are ambiguous")
    assert on_grid.all() and inside.all(), (what, int((~inside).sum()), float(np.abs(q - want).max()))
    assert np.array_equal(lr.astype(np.float32), np.rint(q).astype(np.float32) / np.float32(255))
    return differ
