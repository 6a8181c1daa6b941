"""Host-side mirror of the reference's single-rate model ``WACNN`` (/root/reference/src/compress/models/cnn.py:23-340; "cnn" in the
registry of models/__init__.py) -- the model behind the paper's "base" anchor curve.

Same constructor keywords, method names, argument meaning and return structure as the reference class; the working weights live in HBM
inside the native codec object (pcodec.h: pc_codec_set_model(PC_MODEL_WACNN), pc_codec_wacnn_*), and compress / decompress / forward
are native HIP launch sequences.  Unlike ChannelProgresssiveWACNN's, the y string of compress() is ONE string for the whole batch
(BufferedRansEncoder, cnn.py:236-270): decompress() needs the z strings of the same batch, in the same order.
"""
import ctypes as C

from ._lib import check, lib
from .arch import WacnnConfig, wacnn_param_spec
from .model import _NativeCodecModule, _one_call_at_a_time


class WACNN(_NativeCodecModule):
    """WACNN(N=192, M=320, dim_chunk=32) on the GPU.  A ``torch.nn.Module`` whose tensors are host copies of what was loaded."""

    def __init__(self, N=192, M=320, dim_chunk=32, device="cuda:0", **kwargs):
        super().__init__()
        self.cfg = WacnnConfig(N=N, M=M, dim_chunk=dim_chunk)
        self.cfg.check_supported()                        # before any HIP call
        self.N, self.M, self.dim_chunk = N, M, dim_chunk
        self.num_slices = M // dim_chunk
        self.max_support_slices = 5
        self._open(device)

    @classmethod
    def from_state_dict(cls, state_dict, device="cuda:0"):
        """cnn.py:204-212: always WACNN(192, 320)."""
        net = cls(192, 320, device=device)
        net.load_state_dict(state_dict)
        return net

    def _spec(self):
        return wacnn_param_spec(self.N, self.M, self.dim_chunk)

    def _configure_native(self):
        check(lib().pc_codec_set_model(self._h, 1), "pc_codec_set_model")       # PC_MODEL_WACNN

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("Invalid `inputs` size. Expected a [B,3,H,W] tensor.")
        B, _, H, W = x.shape
        if H % 64 or W % 64:
            raise ValueError("H and W must be multiples of 64 (pad as training/step.py:318 does)")
        return B, H, W

    def _ready(self):
        if self._gc is None or self._eb is None:
            raise ValueError("Uninitialized CDFs. Run update() first")           # entropy_models.py:182-184

    @_one_call_at_a_time
    def compress(self, x):
        """cnn.py:214-271.  Returns {"strings": [[y_string], z_strings], "shape": z.size()[-2:]}: one y string for the batch, one z
        string per image."""
        import torch
        self._ready()
        B, H, W = self._check_input(x)
        x = x.to(self.device, torch.float32).contiguous()
        check(lib().pc_codec_wacnn_compress(self._h, C.c_void_p(x.data_ptr()), B, H, W, self._stream()), "pc_codec_wacnn_compress")
        strs = self._fetch_strings()                                             # the y string, then the B z strings
        return {"strings": [[strs[0]], strs[1:]], "shape": torch.Size([H // 64, W // 64])}

    @_one_call_at_a_time
    def decompress(self, strings, shape):
        """cnn.py:293-340.  strings = [[y_string], z_strings] of ONE compress() call; returns {"x_hat": Tensor[B,3,H,W] in [0,1]}."""
        import torch
        self._ready()
        if not isinstance(strings, (tuple, list)) or len(strings) != 2:
            raise ValueError("Invalid `strings` parameter type.")
        y_strings, z_strings = strings
        if len(y_strings) != 1 or len(z_strings) < 1:
            raise ValueError("Invalid strings or indexes parameters")
        y = bytes(y_strings[0])
        zs = [bytes(s) for s in z_strings]
        B = len(zs)
        zh, zw = int(shape[0]), int(shape[1])
        if zh <= 0 or zw <= 0:
            raise ValueError(f"invalid shape {tuple(shape)}")
        zp = (C.c_char_p * B)(*zs)
        zl = (C.c_size_t * B)(*map(len, zs))
        x_hat = torch.empty((B, 3, 64 * zh, 64 * zw), device=self.device, dtype=torch.float32)
        check(lib().pc_codec_wacnn_decompress(self._h, y, len(y), zp, zl, B, zh, zw, C.c_void_p(x_hat.data_ptr()), self._stream()),
              "pc_codec_wacnn_decompress")
        return {"x_hat": x_hat}

    @_one_call_at_a_time
    def forward(self, x):
        """cnn.py:145-192 in eval mode: {"x_hat": g_s(y_hat) (unclamped), "likelihoods": {"y": [B,320,H/16,W/16], "z": [B,192,H/64,W/64]}};
        y_hat and z_hat are those of compress().  The training-mode (noise) branch is out of scope: a module in training mode (the
        nn.Module default) raises NotImplementedError -- call .eval() first, as the reference's evaluation code does."""
        import torch
        if self.training:
            raise NotImplementedError("only the eval path of WACNN.forward is implemented (call .eval())")
        B, H, W = self._check_input(x)
        x = x.to(self.device, torch.float32).contiguous()
        x_hat = torch.empty((B, 3, H, W), device=self.device, dtype=torch.float32)
        y_lik = torch.empty((B, self.M, H // 16, W // 16), device=self.device, dtype=torch.float32)
        z_lik = torch.empty((B, self.N, H // 64, W // 64), device=self.device, dtype=torch.float32)
        P = lambda t: C.c_void_p(t.data_ptr())
        check(lib().pc_codec_wacnn_forward(self._h, P(x), B, H, W, P(x_hat), P(y_lik), P(z_lik), self._stream()), "pc_codec_wacnn_forward")
        return {"x_hat": x_hat, "likelihoods": {"y": y_lik, "z": z_lik}}
