"""The JPEG stage of the degradation (csrc/jpeg.hip) restated in numpy int64, step for step.  Every intermediate,
and the sum of the magnitudes of every sum's terms (so every partial sum in any order), is asserted to fit int32: what the kernel
computes in int32 is then what this computes in int64, and the GPU tests compare the two bit for bit.  A plain helper module."""
import numpy as np

# Annex K.1 (luminance) and K.2 (chrominance), row = vertical frequency v, column = horizontal frequency u
LUMA = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                 [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                 [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.int64)
CHROMA = np.array([[17, 18, 24, 47, 99, 99, 99, 99], [18, 21, 26, 66, 99, 99, 99, 99], [24, 26, 56, 99, 99, 99, 99, 99],
                   [47, 66, 99, 99, 99, 99, 99, 99]] + [[99] * 8] * 4, np.int64)
MODES = {"444": 0, "420": 1}
TILE = 32                  # the kernel's workgroup tile (pixels); any multiple of 16 gives the same result (tested)
PEAK = [0]                 # the largest magnitude any checked intermediate has reached (the tests print it)


def _i32(a):
    a = np.asarray(a, np.int64)
    if a.size:
        m = int(np.abs(a).max())
        assert m < 2 ** 31, f"an intermediate of magnitude {m} does not fit int32"
        PEAK[0] = max(PEAK[0], m)
    return a


def dct_matrix_f64() -> np.ndarray:
    """The orthonormal 8-point DCT-II matrix C[u][x] in fp64."""
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0] = np.sqrt(0.125)
    return c


def transform_matrix() -> np.ndarray:
    """T[u][x] = rint(8192 C[u][x]), int64 [8, 8]."""
    return np.rint(8192 * dct_matrix_f64()).astype(np.int64)


def tables(Q: int):
    """libjpeg's quality rule on the Annex K tables -> (luminance, chrominance), int64 [8, 8] each, Q in 1..100."""
    assert 1 <= Q <= 100
    s = 5000 // Q if Q < 50 else 200 - 2 * Q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA, CHROMA))


def _sum(spec, t, v):
    """einsum(spec, T, v) with every partial sum inside int32 (the sum of the terms' magnitudes is)."""
    _i32(np.einsum(spec, np.abs(t), np.abs(v)))
    return _i32(np.einsum(spec, t, v))


def _plane_round_trip(plane, q):
    """One plane [8m, 8n] of 0..255 samples through forward DCT, quantiser, dequantiser and inverse DCT -> 0..255."""
    T = transform_matrix()
    m, n = plane.shape[0] // 8, plane.shape[1] // 8
    s = _i32(plane.reshape(m, 8, n, 8).transpose(0, 2, 1, 3) - 128)                 # [m, n, y, x]
    a = _i32((_sum("ux,mnyx->mnyu", T, s) + 512) >> 10)
    F = _sum("vy,mnyu->mnvu", T, a)
    mag = _i32(np.abs(F) + q * 32768) // _i32(q * 65536)
    D = _i32(np.sign(F) * mag * q)
    b = _i32((_sum("vy,mnvu->mnyu", T, D) + 512) >> 10)
    r = _i32((_sum("ux,mnyu->mnyx", T, b) + 32768) >> 16)
    return np.clip(r + 128, 0, 255).transpose(0, 2, 1, 3).reshape(plane.shape)


def _region(x, Q, chroma, y0, x0, side):
    """The pixels [y0, y0 + side) x [x0, x0 + side) of the codec's result on x [3, h, w] (what one workgroup owns): fp32 [3, ny, nx]."""
    _, h, w = x.shape
    M = 16 if chroma else 8
    assert y0 % M == 0 and x0 % M == 0 and side % M == 0
    ny, nx = min(side, -(-(h - y0) // M) * M), min(side, -(-(w - x0) // M) * M)            # whole MCUs
    ys, xs = np.minimum(np.arange(y0, y0 + ny), h - 1), np.minimum(np.arange(x0, x0 + nx), w - 1)     # edge replication
    v = x[:, ys][:, :, xs].astype(np.float32)
    finite = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        c = np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v))              # comparisons: NaN survives
        p = np.where(finite, np.rint(np.float32(255) * c), 0).astype(np.int64)
    bad = ~finite.all(0).reshape(ny // M, M, nx // M, M).all((1, 3))                       # per MCU
    R, G, B = p
    Y = _i32(19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = _i32(-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = _i32(32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    for pl in (Y, Cb, Cr):
        assert pl.min() >= 0 and pl.max() <= 255
    if chroma:
        Cb, Cr = ((pl[0::2, 0::2] + pl[0::2, 1::2] + pl[1::2, 0::2] + pl[1::2, 1::2] + 2) >> 2 for pl in (Cb, Cr))
    ql, qc = tables(Q)
    Y, Cb, Cr = _plane_round_trip(Y, ql), _plane_round_trip(Cb, qc), _plane_round_trip(Cr, qc)
    if chroma:
        Cb, Cr = (pl.repeat(2, 0).repeat(2, 1) for pl in (Cb, Cr))
    Cb, Cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + (_i32(91881 * Cr + 32768) >> 16), Y + (_i32(-22554 * Cb - 46802 * Cr + 32768) >> 16),
                    Y + (_i32(116130 * Cb + 32768) >> 16)])
    out = np.clip(rgb, 0, 255).astype(np.float32) / np.float32(255)
    out[:, bad.repeat(M, 0).repeat(M, 1)] = np.nan
    return out[:, :min(ny, h - y0), :min(nx, w - x0)]


def jpeg_sample(x, Q: int, chroma="420", tile=None) -> np.ndarray:
    """One sample x [3, h, w] fp32 -> fp32 [3, h, w].  tile: None = the image as one piece; a multiple of 16 = cut into tiles of that
    side, each computed on its own (what the kernel's workgroups do with tile = TILE)."""
    x = np.asarray(x, np.float32)
    chroma = MODES[chroma] if isinstance(chroma, str) else int(chroma)
    Q = int(Q)
    if Q == 0:
        return x.copy()
    if Q < 0 or Q > 100:
        return np.full_like(x, np.nan)
    _, h, w = x.shape
    side = tile if tile else -(-max(h, w) // 16) * 16
    out = np.empty_like(x)
    for y0 in range(0, h, side):
        for x0 in range(0, w, side):
            out[:, y0:y0 + side, x0:x0 + side] = _region(x, Q, chroma, y0, x0, side)
    return out


def jpeg_reference(x, deg, chroma="420", tile=None) -> np.ndarray:
    """A batch x [B, 3, h, w] with deg rows int32 [B, 8] (word 6 = Q) -> fp32 [B, 3, h, w]."""
    x, deg = np.asarray(x, np.float32), np.asarray(deg).reshape(len(x), 8)
    return np.stack([jpeg_sample(x[b], int(deg[b, 6]), chroma, tile) for b in range(len(x))])


def same(a, b) -> bool:
    """Bit equality of two fp32 arrays in which every NaN is the same NaN position for position."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def checkerboard(h, w, period=1) -> np.ndarray:
    """[3, h, w] of 0 / 1 squares of `period` pixels, the three channels in different phases."""
    y, x = np.arange(h)[:, None] // period, np.arange(w)[None, :] // period
    return np.stack([(y + x) % 2, (y + x + 1) % 2, (y + 2 * x) % 2]).astype(np.float32)


def fixture_image(H, W, q) -> np.ndarray:
    """The test image of the libjpeg fixtures (tests/golden/make_golden_jpeg.py): uint8 [H, W, 3]."""
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    base = 128 + 70 * np.sin(0.3 * x + 0.2 * y) + 30 * np.cos(0.45 * y - 0.1 * x)
    base = base + 50 * ((y >= H // 3) & (x >= W // 2))
    rng = np.random.default_rng(H * W + q)
    img = np.stack([base, 0.9 * base + 10, 0.8 * base - 5], -1) + rng.normal(0, 4, (H, W, 1)) + rng.normal(0, 1.5, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
