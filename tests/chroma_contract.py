"""The chroma layer (progressivecodec_amd/chroma.py, chroma_hip/pc_chroma.h) restated in numpy from its definition (DESIGN.md section
21), not from the kernels: what tests/test_chroma_host.py checks against tests/frames_contract.py (4:2:0, centre) and against the
float64 formulas, and tests/test_gpu_chroma.py checks the GPU against.  Every float32 product, sum and quotient is one numpy float32
operation; chroma sums and the distortion sums are integers.  What section 21 takes from section 13 unchanged (levels, coefficients,
clamp, rounding) is taken from tests/frames_contract.py.

A frame is a tuple of arrays with a leading batch axis: (Y [B,H,W], UV [B,Hc,Wc,2]) for the semi-planar formats, (Y, U [B,Hc,Wc], V)
for the planar ones; uint8, or uint16 holding code << shift.  Codes are int64 arrays (Y, Cb, Cr).
"""
import numpy as np

from tests import frames_contract as FC

F = np.float32
MATRICES, RANGES, UPSAMPLES = FC.MATRICES, FC.RANGES, FC.UPSAMPLES
coefficients, coefficients64, clamp01, quantise, psnr = FC.coefficients, FC.coefficients64, FC.clamp01, FC.quantise, FC.psnr

# name -> (semi-planar, bits, shift, sx, sy)
FORMATS = {
    "i420": (False, 8, 0, 2, 2), "i422": (False, 8, 0, 2, 1), "i444": (False, 8, 0, 1, 1),
    "nv12": (True, 8, 0, 2, 2), "nv16": (True, 8, 0, 2, 1), "nv24": (True, 8, 0, 1, 1),
    "p010": (True, 10, 6, 2, 2), "p210": (True, 10, 6, 2, 1), "p410": (True, 10, 6, 1, 1),
    "i010": (False, 10, 0, 2, 2), "i210": (False, 10, 0, 2, 1), "i410": (False, 10, 0, 1, 1),
}
# name -> (horizontal, vertical) co-sited?
SITINGS = {"centre": (False, False), "left": (True, False), "topleft": (True, True)}


def bits(fmt):
    return FORMATS[fmt][1]


def sub(fmt):
    return FORMATS[fmt][3:]


def levels(fmt, rng):
    """(yo, ys, co, cs, max code): section 13's, by the bit depth alone"""
    return FC.levels("p010" if bits(fmt) == 10 else "nv12", rng)


def chroma_size(H, W, fmt):
    sx, sy = sub(fmt)
    return -(-H // sy), -(-W // sx)


def codes(planes, fmt):
    """frame -> (Y, Cb, Cr) int64: code = (element >> shift) & (2^bits - 1)"""
    semi, n, sh = FORMATS[fmt][:3]
    get = lambda a: (np.asarray(a).astype(np.int64) >> sh) & (2 ** n - 1)                        # noqa: E731
    if semi:
        uv = get(planes[1])
        return get(planes[0]), uv[..., 0], uv[..., 1]
    return get(planes[0]), get(planes[1]), get(planes[2])


def frame(Y, Cb, Cr, fmt):
    """(Y, Cb, Cr) codes -> frame: element = code << shift"""
    semi, n, sh = FORMATS[fmt][:3]
    dt = np.uint16 if n == 10 else np.uint8
    put = lambda a: np.ascontiguousarray((np.asarray(a, np.int64) << sh).astype(dt))             # noqa: E731
    if semi:
        return put(Y), put(np.stack([Cb, Cr], axis=-1))
    return put(Y), put(Cb), put(Cr)


def taps(r, n, subsampled, linear, cosited):
    """the ingest's two taps ((i0, w0), (i1, w1)) of luma index r on an axis of n chroma samples"""
    if not subsampled:
        return (r, 4), (r, 0)
    i0 = r >> 1
    if not linear:
        return (i0, 4), (i0, 0)
    if not cosited:
        return (i0, 3), (min(max(i0 + (1 if r & 1 else -1), 0), n - 1), 1)
    if r & 1:
        return (i0, 2), (min(i0 + 1, n - 1), 2)
    return (i0, 4), (i0, 0)


def upsample16(C, H, W, fmt, upsample, siting):
    """C int64 [B,Hc,Wc] -> the 16-fold chroma at every luma pixel, int64 [B,H,W]"""
    sx, sy = sub(fmt)
    hco, vco = SITINGS[siting]
    Hc, Wc = C.shape[1:]
    linear = {"nearest": False, "linear": True}[upsample]
    ty = [taps(r, Hc, sy == 2, linear, vco) for r in range(H)]
    tx = [taps(q, Wc, sx == 2, linear, hco) for q in range(W)]
    out = np.zeros((C.shape[0], H, W), np.int64)
    for a in range(2):
        iy, wy = np.array([t[a][0] for t in ty]), np.array([t[a][1] for t in ty])
        for b in range(2):
            jx, wx = np.array([t[b][0] for t in tx]), np.array([t[b][1] for t in tx])
            out += wy[None, :, None] * wx[None, None, :] * C[:, iy][:, :, jx]
    return out


def rgb(planes, fmt, matrix, rng, upsample, siting):
    """frame -> float32 [B,3,H,W]"""
    yo, ys, co, cs, _ = levels(fmt, rng)
    a, b, c, d = coefficients(matrix)[:4]
    Y, Cb, Cr = codes(planes, fmt)
    H, W = Y.shape[1:]
    y = (Y - yo).astype(F) / F(ys)
    cb = (upsample16(Cb, H, W, fmt, upsample, siting) - 16 * co).astype(F) / F(16 * cs)
    cr = (upsample16(Cr, H, W, fmt, upsample, siting) - 16 * co).astype(F) / F(16 * cs)
    R = y + (cr * a)
    G = (y - (cb * b)) - (cr * c)
    Bl = y + (cb * d)
    assert R.dtype == G.dtype == Bl.dtype == F
    return np.stack([clamp01(R), clamp01(G), clamp01(Bl)], axis=1)


def ingest(planes, fmt, matrix, rng, upsample, siting, hp, wp, top, left):
    x = rgb(planes, fmt, matrix, rng, upsample, siting)
    B, _, H, W = x.shape
    out = np.zeros((B, 3, hp, wp), F)
    out[:, :, top:top + H, left:left + W] = x
    return out


def axis_filter(p, axis, subsampled, cosited):
    """the emit's per-axis rule on float32 p along `axis` (N luma samples) -> (h with ceil(N / 2) or N samples, scale)"""
    if not subsampled:
        return p, 1
    N = p.shape[axis]
    j = np.arange(-(-N // 2))
    take = lambda idx: np.take(p, idx, axis=axis)                                                # noqa: E731
    b, c = take(2 * j), take(np.minimum(2 * j + 1, N - 1))
    if not cosited:
        h, scale = b + c, 2
    else:
        a = take(np.maximum(2 * j - 1, 0))
        h, scale = (a + c) + (b + b), 4
    assert h.dtype == F
    return h, scale


def emit_parts(x, top, left, H, W, fmt, matrix, rng, siting):
    """x float32 [B,3,Hp,Wp] -> (Y codes, [v_b, v_r] float32 filtered differences before the scale, s)"""
    yo, ys, co, cs, mx = levels(fmt, rng)
    kr, kg, kb, ib, ir = coefficients(matrix)[4:]
    sx, sy = sub(fmt)
    hco, vco = SITINGS[siting]
    c = clamp01(x[:, :, top:top + H, left:left + W])
    R, G, Bl = c[:, 0], c[:, 1], c[:, 2]
    Yf = ((kr * R) + (kg * G)) + (kb * Bl)
    Cb, Cr = (Bl - Yf) * ib, (R - Yf) * ir
    Y = quantise((Yf * F(ys)) + F(yo), mx)
    vs = []
    for Cp in (Cb, Cr):
        u = Cp * F(cs)
        assert u.dtype == F
        h, sh = axis_filter(u, 2, sx == 2, hco)                   # along rows first
        v, sv = axis_filter(h, 1, sy == 2, vco)                   # then along columns
        vs.append(v)
    return Y, vs, F(1.0 / (sh * sv))


def emit_codes(x, top, left, H, W, fmt, matrix, rng, siting):
    """x float32 [B,3,Hp,Wp] -> (Y, Cb, Cr) int64"""
    _, _, co, _, mx = levels(fmt, rng)
    Y, vs, s = emit_parts(x, top, left, H, W, fmt, matrix, rng, siting)
    out = [Y]
    for v in vs:
        m = v * s + F(co)
        assert m.dtype == F
        out.append(quantise(m, mx))
    return tuple(out)


def emit(x, top, left, H, W, fmt, matrix, rng, siting):
    return frame(*emit_codes(x, top, left, H, W, fmt, matrix, rng, siting), fmt)


def sums(x, top, left, H, W, fmt, matrix, rng, siting, ref):
    """[B][3] Python ints: per frame and plane [Y, Cb, Cr] the sum of (code - refcode)^2"""
    got, want = emit_codes(x, top, left, H, W, fmt, matrix, rng, siting), codes(ref, fmt)
    B = x.shape[0]
    return [[int(((g[b] - w[b]) ** 2).sum()) for g, w in zip(got, want)] for b in range(B)]


def random_frame(B, H, W, fmt, seed, garbage=False):
    """seeded random codes over the whole code range; garbage: the bits of a 16-bit word outside the code are random, too"""
    rng = np.random.default_rng(seed)
    semi, n, sh = FORMATS[fmt][:3]
    Hc, Wc = chroma_size(H, W, fmt)
    planes = frame(*[rng.integers(0, 2 ** n, shape, dtype=np.int64) for shape in ((B, H, W), (B, Hc, Wc), (B, Hc, Wc))], fmt)
    if garbage and n == 10:
        keep = np.uint16((2 ** n - 1) << sh)
        planes = tuple((p & keep) | (rng.integers(0, 2 ** 16, p.shape).astype(np.uint16) & ~keep) for p in planes)
    return planes


def hostile_planes(planes, fmt, matrix, rng, siting, hp, wp, top, left, seed):
    """Decoder-like planes for an emit test: the ingest of a frame plus noise, with values below 0, above 1, +-inf, NaN and -0.0
    sprinkled over it, padding included (frames_contract.hostile_planes for any format)."""
    g = np.random.default_rng(seed)
    x = ingest(planes, fmt, matrix, rng, "linear", siting, hp, wp, top, left)
    x = (x + g.normal(0, 0.05, x.shape).astype(F)).astype(F)
    flat = x.reshape(-1)
    special = np.array([-0.0, 0.0, 1.0, -1.5, 2.5, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.5, 1 - 2.0 ** -24], F)
    n = min(flat.size, max(len(special), flat.size // 7))
    idx = g.choice(flat.size, n, replace=False)
    flat[idx] = special[np.arange(n) % len(special)]
    return x
