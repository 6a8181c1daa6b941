"""The checker for progressivecodec_amd.metrics: the definition of DESIGN.md section 9 (the public behaviour of pytorch_msssim 1.0
ssim / ms_ssim; Wang, Simoncelli, Bovik 2003) restated in float64 torch ops on the CPU.  Not product code."""
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss_1d(win_size=11, sigma=1.5):
    """the window, built in float32 as the library builds it, normalised to sum 1"""
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def gaussian_filter(x, g):
    """separable valid filter per channel: first along H, then along W"""
    C = x.shape[1]
    n = g.numel()
    g = g.to(x.dtype)
    x = F.conv2d(x, g.view(1, 1, n, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, n).repeat(C, 1, 1, 1), groups=C)


def pool2(x):
    """avg_pool2d(2, 2) with a zero on both sides of an odd dimension, divisor 4"""
    return F.avg_pool2d(x, kernel_size=2, stride=2, padding=(x.shape[2] % 2, x.shape[3] % 2))


def ssim_per_channel(X, Y, data_range, g, K=(0.01, 0.03)):
    """(ssim_c, cs_c): the means of the two maps per (image, channel), [B, C]"""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = gaussian_filter(X, g), gaussian_filter(Y, g)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = gaussian_filter(X * X, g) - mu1_sq
    s2 = gaussian_filter(Y * Y, g) - mu2_sq
    s12 = gaussian_filter(X * Y, g) - mu12
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim_ref(X, Y, data_range=255, win_size=11, win_sigma=1.5, weights=MS_WEIGHTS, K=(0.01, 0.03), scales=False):
    """per-image MS-SSIM [B] (float64); with scales=True also the per-scale (ssim_c, cs_c) list"""
    X, Y = X.double().cpu(), Y.double().cpu()
    assert min(X.shape[2:]) > (win_size - 1) * 16
    g = gauss_1d(win_size, win_sigma)
    w = torch.tensor(weights, dtype=torch.float64)
    per = []
    for i in range(len(weights)):
        s, cs = ssim_per_channel(X, Y, data_range, g, K)
        per.append((s, cs))
        if i < len(weights) - 1:
            X, Y = pool2(X), pool2(Y)
    m = torch.stack([torch.relu(cs) for _, cs in per[:-1]] + [torch.relu(per[-1][0])])
    val = torch.prod(m ** w.view(-1, 1, 1), dim=0).mean(1)
    return (val, per) if scales else val


def ssim_ref(X, Y, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """per-image SSIM [B] (float64)"""
    X, Y = X.double().cpu(), Y.double().cpu()
    s, _ = ssim_per_channel(X, Y, data_range, gauss_1d(win_size, win_sigma), K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean(1)
