"""The UNet post-filter (reference layers/unet.py, CHProg_cnn.py:277-284) restated on the numeric contract of DESIGN.md section 2, for the
tests only -- product code never imports this file.  Every conv is the CPU oracle's fmaf chain (oracle.liboracle.conv_nhwc) plus its
bias; sigmoid is the contract's (oracle.liboracle.unary); ReLU, LeakyReLU, the SE scale-add, the residual adds and max-pool are single
float32 numpy operations; the SE mean follows the documented summation order:

  chunks of 4096 pixels; in a chunk, G = 1024 / C pixel groups, group g summing pixels g, g + G, ... in ascending order from +0; the G
  group sums added in ascending g from +0; the chunk sums added in ascending chunk order from +0; divided by H*W (one rounding).
"""
import numpy as np

from oracle.liboracle import conv_nhwc, unary

F32 = np.float32
SE_CHUNK = 4096


def refine_weights(sd, prefix):
    """{name: float32 array} of Sequential(UNet(3, 16), conv3x3(16, 3)) under `prefix` ("refine" / "refine.0" / "refine.1")."""
    p = prefix + "."
    return {k[len(p):]: np.asarray(v.numpy() if hasattr(v, "numpy") else v, F32) for k, v in sd.items() if k.startswith(p)}


def conv(x, w, b, k):
    """'same' conv, stride 1: x NHWC, w [Cout][Cin][k][k] (nn.Conv2d), + bias"""
    B, H, W, _ = x.shape
    taps = [(ky - k // 2, kx - k // 2) for ky in range(k) for kx in range(k)]
    wt = np.ascontiguousarray(np.transpose(w, (2, 3, 1, 0)).reshape(k * k, w.shape[1], w.shape[0]))
    return conv_nhwc(x, wt, taps, 1, H, W) + b.astype(F32)


def leaky(v):
    return np.where(v > 0, v, v * F32(0.01)).astype(F32)


def relu(v):
    return np.where(v > 0, v, F32(0.0)).astype(F32)


def se_mean(t):
    """t NHWC [B,H,W,C] -> [B,C] in the documented order"""
    B, H, W, C = t.shape
    HW = H * W
    G = 1024 // C
    nchunk = (HW + SE_CHUNK - 1) // SE_CHUNK
    x = np.zeros((B, nchunk * SE_CHUNK, C), F32)        # zero tail: adding +0 to a chain that never holds -0 changes nothing
    x[:, :HW] = t.reshape(B, HW, C)
    x = x.reshape(B, nchunk, SE_CHUNK // G, G, C)
    acc = np.zeros((B, nchunk, G, C), F32)
    for i in range(SE_CHUNK // G):
        acc = acc + x[:, :, i]
    chunk = np.zeros((B, nchunk, C), F32)
    for g in range(G):
        chunk = chunk + acc[:, :, g]
    tot = np.zeros((B, C), F32)
    for k in range(nchunk):
        tot = tot + chunk[:, k]
    return (tot / F32(HW)).astype(F32)


def se_scale(t, fc1, fc2):
    """SELayer.fc on the mean (unet.py:37-47): Linear(C, C/16) -> ReLU -> Linear(C/16, C) -> sigmoid, the Linears as contract chains"""
    m = se_mean(t)
    B, C = m.shape
    h = conv_nhwc(m.reshape(B, 1, 1, C), np.ascontiguousarray(fc1.T)[None], [(0, 0)], 1, 1, 1)
    h = relu(h)
    z = conv_nhwc(h, np.ascontiguousarray(fc2.T)[None], [(0, 0)], 1, 1, 1)
    return unary(z.reshape(B, C), "sigmoid")


def cbr(x, w, p):
    """ConvBlockResidual (unet.py:55-70): up_dim(x) + SE(conv3x3(leaky(conv3x3(x))))"""
    t = leaky(conv(x, w[p + ".conv.0.weight"], w[p + ".conv.0.bias"], 3))
    t = conv(t, w[p + ".conv.2.weight"], w[p + ".conv.2.bias"], 3)
    s = se_scale(t, w[p + ".conv.3.fc.0.weight"], w[p + ".conv.3.fc.2.weight"])
    u = conv(x, w[p + ".up_dim.weight"], w[p + ".up_dim.bias"], 1)
    return (u + t * s[:, None, None, :]).astype(F32)


def maxpool2(x):
    """MaxPool2d(2): the window visited (0,0) (0,1) (1,0) (1,1), a value replaces the running max when larger or NaN"""
    v = [x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]]
    m = v[0]
    for a in v[1:]:
        m = np.where((a > m) | np.isnan(a), a, m)
    return m.astype(F32)


def up_ps(x, w, b):
    """subpel_conv1x1(., ., 2): 1x1 conv then PixelShuffle(2)"""
    y = conv(x, w, b, 1)
    B, H, W, C4 = y.shape
    y = y.reshape(B, H, W, C4 // 4, 2, 2).transpose(0, 1, 4, 2, 5, 3)
    return np.ascontiguousarray(y.reshape(B, 2 * H, 2 * W, C4 // 4))


def refine(x_nchw, w, clamp=False):
    """Sequential(UNet(3, 16), conv3x3(16, 3)) on NCHW float32; clamp: the decode paths' clamp_(0, 1) of the result"""
    x = np.ascontiguousarray(np.asarray(x_nchw, F32).transpose(0, 2, 3, 1))
    u = "0."
    x1 = cbr(x, w, u + "conv1")
    x2 = cbr(maxpool2(x1), w, u + "conv2")
    x3 = cbr(maxpool2(x2), w, u + "conv3")
    for i in range(4):
        p = f"{u}context_refine.{i}"
        t = relu(conv(relu(x3), w[p + ".conv1.weight"], w[p + ".conv1.bias"], 3))
        t = conv(t, w[p + ".conv2.weight"], w[p + ".conv2.bias"], 3)
        x3 = (x3 + t).astype(F32)
    d3 = up_ps(x3, w[u + "up3.0.weight"], w[u + "up3.0.bias"])
    d3 = cbr(np.concatenate([x2, d3], axis=3), w, u + "up_conv3")
    d2 = up_ps(d3, w[u + "up2.0.weight"], w[u + "up2.0.bias"])
    d2 = cbr(np.concatenate([x1, d2], axis=3), w, u + "up_conv2")
    y = conv(d2, w["1.weight"], w["1.bias"], 3)
    if clamp:
        y = np.where(y < 0, F32(0), np.where(y > 1, F32(1), y)).astype(F32)
    return np.ascontiguousarray(y.transpose(0, 3, 1, 2))
