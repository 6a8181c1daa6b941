"""The YUV 4:2:0 layer (progressivecodec_amd/frames.py, frames_csrc/pc_frames.h) restated in numpy from its definition (DESIGN.md
section 13), not from the kernels: what tests/test_frames_host.py checks against the float64 formulas and tests/test_gpu_frames.py
checks the GPU against.  Every float32 product, sum and quotient is one numpy float32 operation; chroma and the sums are integers.

A frame is a tuple of arrays with a leading batch axis: (Y [B,H,W], UV [B,Hc,Wc,2]) for "nv12" (uint8) and "p010" (uint16, code << 6),
(Y, U [B,Hc,Wc], V) for "i420" (uint8).  Codes are int64 arrays (Y, Cb, Cr).
"""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
FORMATS = ("nv12", "i420", "p010")
RANGES = ("limited", "full")
UPSAMPLES = ("nearest", "linear")
F = np.float32


def bits(fmt):
    return {"nv12": 8, "i420": 8, "p010": 10}[fmt]


def levels(fmt, rng):
    """(yo, ys, co, cs, max code)"""
    n = bits(fmt)
    s, top = 2 ** (n - 8), 2 ** n - 1
    return {"limited": (16 * s, 219 * s, 128 * s, 224 * s, top), "full": (0, top, 128 * s, top, top)}[rng]


def coefficients64(matrix):
    """a, b, c, d, Kr, Kg, Kb, ib, ir in float64"""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    return (2 * (1 - kr), 2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg, 2 * (1 - kb), kr, kg, kb, 1 / (2 * (1 - kb)), 1 / (2 * (1 - kr)))


def coefficients(matrix):
    """the same nine, each rounded once to float32"""
    return tuple(F(v) for v in coefficients64(matrix))


def chroma_size(H, W):
    return -(-H // 2), -(-W // 2)


def codes(planes, fmt):
    """frame -> (Y, Cb, Cr) int64"""
    sh = 6 if fmt == "p010" else 0
    y = np.asarray(planes[0]).astype(np.int64) >> sh
    if fmt == "i420":
        return y, np.asarray(planes[1]).astype(np.int64), np.asarray(planes[2]).astype(np.int64)
    uv = np.asarray(planes[1]).astype(np.int64) >> sh
    return y, uv[..., 0], uv[..., 1]


def frame(Y, Cb, Cr, fmt):
    """(Y, Cb, Cr) codes -> frame"""
    if fmt == "i420":
        return tuple(np.ascontiguousarray(a.astype(np.uint8)) for a in (Y, Cb, Cr))
    dt, sh = (np.uint16, 6) if fmt == "p010" else (np.uint8, 0)
    return (Y << sh).astype(dt), (np.stack([Cb, Cr], axis=-1) << sh).astype(dt)


def taps(r, n):
    """the two chroma indices (near, far) of luma index r on an axis of n chroma samples"""
    i0 = r >> 1
    return i0, min(max(i0 + (1 if r & 1 else -1), 0), n - 1)


def upsample16(C, H, W, upsample):
    """C int64 [B,Hc,Wc] -> the 16-fold chroma at every luma pixel, int64 [B,H,W]"""
    Hc, Wc = C.shape[1:]
    i0, i1 = np.array([taps(r, Hc) for r in range(H)]).T
    j0, j1 = np.array([taps(q, Wc) for q in range(W)]).T
    if upsample == "nearest":
        return 16 * C[:, i0][:, :, j0]
    if upsample != "linear":
        raise ValueError(upsample)
    return 9 * C[:, i0][:, :, j0] + 3 * C[:, i0][:, :, j1] + 3 * C[:, i1][:, :, j0] + C[:, i1][:, :, j1]


def clamp01(v):
    """fminf(fmaxf(v, 0), 1): NaN -> 0"""
    return np.fmin(np.fmax(np.asarray(v, F), F(0)), F(1))


def rgb(planes, fmt, matrix, rng, upsample):
    """frame -> float32 [B,3,H,W]"""
    yo, ys, co, cs, _ = levels(fmt, rng)
    a, b, c, d = coefficients(matrix)[:4]
    Y, Cb, Cr = codes(planes, fmt)
    H, W = Y.shape[1:]
    y = (Y - yo).astype(F) / F(ys)
    cb = (upsample16(Cb, H, W, upsample) - 16 * co).astype(F) / F(16 * cs)
    cr = (upsample16(Cr, H, W, upsample) - 16 * co).astype(F) / F(16 * cs)
    R = y + (cr * a)
    G = (y - (cb * b)) - (cr * c)
    Bl = y + (cb * d)
    assert R.dtype == G.dtype == Bl.dtype == F
    return np.stack([clamp01(R), clamp01(G), clamp01(Bl)], axis=1)


def ingest(planes, fmt, matrix, rng, upsample, hp, wp, top, left):
    x = rgb(planes, fmt, matrix, rng, upsample)
    B, _, H, W = x.shape
    out = np.zeros((B, 3, hp, wp), F)
    out[:, :, top:top + H, left:left + W] = x
    return out


def quantise(v, top):
    """clampi(rintf(v), 0, top) of finite float32 values"""
    return np.clip(np.rint(v).astype(np.int64), 0, top)


def emit_codes(x, top, left, H, W, fmt, matrix, rng):
    """x float32 [B,3,Hp,Wp] -> (Y, Cb, Cr) int64"""
    yo, ys, co, cs, mx = levels(fmt, rng)
    kr, kg, kb, ib, ir = coefficients(matrix)[4:]
    c = clamp01(x[:, :, top:top + H, left:left + W])
    R, G, Bl = c[:, 0], c[:, 1], c[:, 2]
    Yf = ((kr * R) + (kg * G)) + (kb * Bl)
    Cb, Cr = (Bl - Yf) * ib, (R - Yf) * ir
    Y = quantise((Yf * F(ys)) + F(yo), mx)
    out = [Y]
    for Cp in (Cb, Cr):
        u = Cp * F(cs)
        assert u.dtype == F
        u = np.pad(u, ((0, 0), (0, H & 1), (0, W & 1)), mode="edge")          # rows min(2i+1, H-1), columns min(2j+1, W-1)
        m = ((u[:, 0::2, 0::2] + u[:, 0::2, 1::2]) + (u[:, 1::2, 0::2] + u[:, 1::2, 1::2])) * F(0.25) + F(co)
        assert m.dtype == F
        out.append(quantise(m, mx))
    return tuple(out)


def emit(x, top, left, H, W, fmt, matrix, rng):
    return frame(*emit_codes(x, top, left, H, W, fmt, matrix, rng), fmt)


def sums(x, top, left, H, W, fmt, matrix, rng, ref):
    """[B][3] Python ints: per frame and plane [Y, Cb, Cr] the sum of (code - refcode)^2"""
    got, want = emit_codes(x, top, left, H, W, fmt, matrix, rng), codes(ref, fmt)
    B = x.shape[0]
    return [[int(((g[b] - w[b]) ** 2).sum()) for g, w in zip(got, want)] for b in range(B)]


def psnr(sse, n, peak):
    import math
    return 10.0 * math.log10(float(peak) ** 2 * n / sse) if sse > 0 else float("inf")


def relayout(planes, fmt, to):
    """the same codes in another layout of the same bit depth"""
    return frame(*codes(planes, fmt), to)


def random_frame(B, H, W, fmt, seed):
    """seeded random codes over the whole code range (reserved codes included), every code value present where there is room"""
    rng = np.random.default_rng(seed)
    top = 2 ** bits(fmt)
    Hc, Wc = chroma_size(H, W)
    out = []
    for shape in ((B, H, W), (B, Hc, Wc), (B, Hc, Wc)):
        a = rng.integers(0, top, shape, dtype=np.int64)
        flat = a.reshape(-1)
        n = min(top, flat.size)
        flat[rng.permutation(flat.size)[:n]] = np.arange(n)
        out.append(a)
    return frame(*out, fmt)


def hostile_planes(planes, fmt, matrix, rng, hp, wp, top, left, seed):
    """Decoder-like planes for an emit test: the ingest of a frame plus noise, with values below 0, above 1, +-inf, NaN and -0.0
    sprinkled over it, padding included."""
    g = np.random.default_rng(seed)
    x = ingest(planes, fmt, matrix, rng, "linear", hp, wp, top, left)
    x = (x + g.normal(0, 0.05, x.shape).astype(F)).astype(F)
    flat = x.reshape(-1)
    special = np.array([-0.0, 0.0, 1.0, -1.5, 2.5, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.5, 1 - 2.0 ** -24], F)
    n = min(flat.size, max(len(special), flat.size // 7))
    idx = g.choice(flat.size, n, replace=False)
    flat[idx] = special[np.arange(n) % len(special)]
    return x
