"""The reference's single-rate model WACNN (models/cnn.py:23-340) restated over the oracle's blocks, for the tests only -- product code
never imports this file.  Back-end "torch" follows the reference's own ATen operations, whose rounding depends on the CPU's oneDNN
kernels (tests/test_wacnn_host.py holds it to the reference within rounding); back-end "cdet" follows the numeric contract of DESIGN.md
section 2, is the same on every CPU, reproduces the reference's strings in the golden cases, and is what the GPU reproduces bit for bit.

WACNN's layers are those of ChannelProgresssiveWACNN's base path, so RefCodec's g_a (one 3 -> 320 net), h_a, stack5 and LRP run
unchanged; only two places differ in their keys -- g_s.<layer> and h_{mean,scale}_s.<layer> carry no ModuleList index -- and the
framing: every symbol of every slice and image goes into ONE rANS stream (BufferedRansEncoder, cnn.py:236-270) in the order
[slice][B][32][h][w], decoded back with one decode_stream per slice (cnn.py:314-332).
"""
import numpy as np
import torch

from oracle import liboracle as lo
from oracle.codec_ref import MAX_SUPPORT, RefCodec
from progressivecodec_amd import entropy

NS = 10


class WacnnCodec(RefCodec):
    def g_s(self, y):                                   # cnn.py:45-55 (unclamped)
        d = lambda x, q: self.ops.deconv(x, self.sd[q + ".weight"], self.sd[q + ".bias"])
        x = self._wam(y, "g_s.0", 4, 2)
        x = self._gdn(d(x, "g_s.1"), "g_s.2", True)
        x = self._gdn(d(x, "g_s.3"), "g_s.4", True)
        x = self._wam(x, "g_s.5", 8, 4)
        x = self._gdn(d(x, "g_s.6"), "g_s.7", True)
        return d(x, "g_s.8")

    def _h_s(self, p, z):                               # cnn.py:69-91 (h_mean_s / h_scale_s)
        g = self.ops.gelu
        x = g(self._c(z, p + ".0"))
        x = g(torch.nn.functional.pixel_shuffle(self._c(x, p + ".2.0"), 2))
        x = g(self._c(x, p + ".4"))
        x = g(torch.nn.functional.pixel_shuffle(self._c(x, p + ".6.0"), 2))
        return self._c(x, p + ".8")

    def _chain(self, y, lm, ls, code):
        """the ten slices (cnn.py:237-266); code(i, mu, scale, idx, y_slice) -> symbols [B,32,h,w] int32.  Returns y_hat and per-slice taps."""
        y_slices = y.chunk(NS, 1) if y is not None else [None] * NS
        y_hat, taps = [], []
        for i in range(NS):
            sup = y_hat[:min(MAX_SUPPORT, i)]
            mean_support = torch.cat([lm] + sup, 1)
            mu = self.stack5("cc_mean_transforms", i, mean_support)
            scale = self.stack5("cc_scale_transforms", i, torch.cat([ls] + sup, 1))
            idx = self._indexes(scale)                                      # build_indexes :250
            sym = code(i, mu, scale, idx, y_slices[i])
            yh = self._lrp("lrp_transforms", i, mean_support, sym.float() + mu)   # :252, :258-261
            y_hat.append(yh)
            taps.append(dict(mu=mu, scale=scale, idx=idx, sym=sym))
        return torch.cat(y_hat, 1), taps

    def _front(self, x):
        y = self._g_a_net(x, "g_a")                                         # :215
        z = self.h_a(y)                                                     # :218
        med = self.medians.view(1, -1, 1, 1)
        z_sym = torch.from_numpy(lo.quantize(z.numpy(), med.expand_as(z).contiguous().numpy()))
        z_hat = z_sym.float() + med                                         # :219-220
        return y, z, z_sym, z_hat

    def compress(self, x):
        """cnn.py:214-271 -> {"strings": [[y_string], z_strings], "shape"}"""
        y, z, z_sym, z_hat = self._front(x)
        B, _, zh, zw = z.shape
        z_strings = self._encode(z_sym, self._eb_indexes(B, zh, zw), self.eb)
        lm, ls = self._h_s("h_mean_s", z_hat), self._h_s("h_scale_s", z_hat)
        code = lambda i, mu, scale, idx, ys: torch.from_numpy(lo.quantize(ys.numpy(), mu.numpy()))
        _, taps = self._chain(y, lm, ls, code)
        sym = np.concatenate([t["sym"].numpy().reshape(-1) for t in taps])   # slice-major, then image, then C,H,W
        idx = np.concatenate([t["idx"].numpy().reshape(-1) for t in taps])
        return {"strings": [[lo.rans_encode(sym, idx, self.gc)], z_strings], "shape": torch.Size([zh, zw])}

    def decompress(self, strings, shape):
        """cnn.py:293-340 -> {"x_hat"} clamped"""
        y_strings, z_strings = strings
        B = len(z_strings)
        zh, zw = int(shape[0]), int(shape[1])
        med = self.medians.view(1, -1, 1, 1)
        z_hat = self._decode(z_strings, self._eb_indexes(B, zh, zw), self.eb).float() + med
        lm, ls = self._h_s("h_mean_s", z_hat), self._h_s("h_scale_s", z_hat)
        dec = entropy.RansDecoder()
        dec.set_stream(y_strings[0])
        tab = entropy.CdfTables(self.gc.cdf, self.gc.length, self.gc.offset)

        def code(i, mu, scale, idx, ys):
            rv = dec.decode_stream(idx.numpy().reshape(-1), tab, None, None)
            return torch.tensor(rv, dtype=torch.int32).reshape(mu.shape)
        y_hat, _ = self._chain(None, lm, ls, code)
        return {"x_hat": self.g_s(y_hat).clamp_(0, 1)}

    def forward(self, x):
        """cnn.py:145-192 in eval mode -> {"x_hat" (unclamped), "likelihoods": {"y", "z"}}"""
        y, z, z_sym, z_hat = self._front(x)
        z_lik = self._eb_likelihood(z_hat)
        lm, ls = self._h_s("h_mean_s", z_hat), self._h_s("h_scale_s", z_hat)
        code = lambda i, mu, scale, idx, ys: torch.from_numpy(lo.quantize(ys.numpy(), mu.numpy()))
        y_hat, taps = self._chain(y, lm, ls, code)
        liks = [self._gc_likelihood(t["sym"].float() + t["mu"] - t["mu"], t["scale"]) for t in taps]
        return {"x_hat": self.g_s(y_hat), "likelihoods": {"y": torch.cat(liks, 1), "z": z_lik}}
