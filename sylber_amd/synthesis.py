"""``SegmentSynthesis.resynthesize`` on the MI355X (sylber/model/segment_synthesis.py:57-146): HuBERT hidden states
(``HubertEncoderHIP``) -> segmentation (``HubertEncoderHIP.segment``) -> segment-mean conditioning (``SegmentConditioner``)
-> the flow-matching decoder (``CfmDecoder``, csrc/cfm.hip: sylber/model/flowmatching.py:474-824) -> the 14-channel
articulatory trajectory ``art``.

The decoder only exists at the sylber_resynthesis.yaml geometry; any other raises ``ValueError``.  Training (``forward``,
the loss, the ``Thresholder`` updates), the torchode path and classifier-free guidance (``cond_scale != 1``) are not here:
upstream's ``resynthesize`` uses none of them."""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .downstream import LEARNED_QUANTIZER_NO_FEATURES, KMQuantizer, ResidualKMQuantizer, SegmentConditioner, quantizer_codebooks
from .quantizer import Quantizer
from .segmenter import PACKED_PRECISIONS, HubertEncoderHIP, _segment_list, _tables_to_host
from .weights import (CFM_CONV_K, CFM_DEPTH, CFM_DIM, CFM_DIM_COND_EMB, CFM_DIM_HEAD, CFM_DIM_IN_PROJ, CFM_DIM_OUT, CFM_FF_INNER,
                      CFM_FF_MULT, CFM_HEADS, CFM_REGISTERS, CFM_TIME_HIDDEN)

PRECISIONS = {"bf16": 0, "fp32": 1, "fp16": 3}        # include/sylber_hip.h SYLBER_BF16 / SYLBER_FP32 / SYLBER_FP16

# sylber_configs/sylber_resynthesis.yaml
DEFAULT_INPUT_CONFIGS = {"output_dim": 256, "hidden_dims": [512, 512], "dropout": 0.05}
DEFAULT_REGRESSOR_CONFIGS = {"depth": 8, "sigma": 0.0, "dim_head": 64, "heads": 8, "dim": 512, "dim_in_proj": 64, "dim_cond_emb": 256}
DEFAULT_THRESHOLDER_CONFIGS = {"signal_mean": 6.10, "signal_var": 0.87, "noise_mean": 0.3879, "noise_var": 0.6819}

# the Regressor's constructor arguments the decoder is built for, with flowmatching.py's defaults where the yaml is silent
_GEOMETRY = {"dim": CFM_DIM, "depth": CFM_DEPTH, "heads": CFM_HEADS, "dim_head": CFM_DIM_HEAD, "dim_in_proj": CFM_DIM_IN_PROJ,
             "dim_cond_emb": CFM_DIM_COND_EMB, "dim_out": CFM_DIM_OUT, "num_register_tokens": CFM_REGISTERS,
             "conv_pos_embed_kernel_size": CFM_CONV_K, "ff_mult": CFM_FF_MULT, "time_hidden_dim": CFM_TIME_HIDDEN}
_NOT_SUPPORTED = {"use_gateloop_layers": False, "conv_pos_embed_groups": None, "attn_qk_norm": True, "condition_on_text": True}


def regressor_shapes() -> Dict[str, tuple]:
    """tensor shapes of ``Regressor.state_dict()`` the decoder reads, at the supported geometry"""
    D, HD, TH, FI = CFM_DIM, CFM_HEADS * CFM_DIM_HEAD, CFM_TIME_HIDDEN, CFM_FF_INNER
    s = {"proj_in.weight": (CFM_DIM_IN_PROJ, CFM_DIM_OUT), "proj_in.bias": (CFM_DIM_IN_PROJ,),
         "sinu_pos_emb.0.weights": (D // 2,), "sinu_pos_emb.1.weight": (TH, D), "sinu_pos_emb.1.bias": (TH,),
         "to_embed.weight": (D, 2 * CFM_DIM_IN_PROJ + CFM_DIM_COND_EMB), "to_embed.bias": (D,),
         "conv_embed.dw_conv1d.0.weight": (D, 1, CFM_CONV_K), "conv_embed.dw_conv1d.0.bias": (D,),
         "transformer.register_tokens": (CFM_REGISTERS, D), "transformer.rotary_emb.inv_freq": (CFM_DIM_HEAD // 2,),
         "transformer.final_norm.gamma": (D,), "to_pred.weight": (CFM_DIM_OUT, D)}
    for i in range(CFM_DEPTH):
        p = "transformer.layers.%d." % i
        for n in (2, 4):
            s[p + "%d.to_gamma.weight" % n] = s[p + "%d.to_beta.weight" % n] = (D, TH)
            s[p + "%d.to_gamma.bias" % n] = s[p + "%d.to_beta.bias" % n] = (D,)
        s[p + "3.q_norm.gamma"] = s[p + "3.k_norm.gamma"] = (CFM_HEADS, 1, CFM_DIM_HEAD)
        s[p + "3.to_qkv.weight"] = (3 * HD, D)
        s[p + "3.to_out.weight"] = (D, HD)
        s[p + "5.0.weight"] = (2 * FI, D)
        s[p + "5.0.bias"] = (2 * FI,)
        s[p + "5.3.weight"] = (D, FI)
        s[p + "5.3.bias"] = (D,)
    return s


def check_regressor_configs(cfg: Optional[dict]) -> None:
    """``ValueError`` unless ``regressor_configs`` describes the geometry the decoder is built for"""
    cfg = dict(cfg or {})
    for k, v in cfg.items():
        if k in _GEOMETRY and int(v) != _GEOMETRY[k]:
            raise ValueError("regressor_configs[%r] = %r: the HIP decoder is built for %s = %d only (sylber_resynthesis.yaml)"
                             % (k, v, k, _GEOMETRY[k]))
        if k in _NOT_SUPPORTED and v != _NOT_SUPPORTED[k]:
            raise ValueError("regressor_configs[%r] = %r is not supported by the HIP decoder" % (k, v))
    if "dim" in cfg and "time_hidden_dim" not in cfg and int(cfg["dim"]) * 4 != CFM_TIME_HIDDEN:
        raise ValueError("time_hidden_dim must be %d" % CFM_TIME_HIDDEN)


def _strip(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def unwrap_checkpoint(ckpt) -> Dict[str, torch.Tensor]:
    """path (``torch.load``) or dict; a Lightning ``{"state_dict": {"net.<key>": ...}}`` wrapper is unwrapped to the keys of
    ``SegmentSynthesis.state_dict()``"""
    if isinstance(ckpt, (str, Path)):
        ckpt = torch.load(str(ckpt), map_location="cpu")
    if not isinstance(ckpt, dict):
        raise TypeError("model_ckpt must be a path or a state dict")
    if "state_dict" in ckpt and isinstance(ckpt["state_dict"], dict):
        ckpt = ckpt["state_dict"]
    if any(k.startswith("net.") for k in ckpt):
        ckpt = _strip(ckpt, "net.")
    return ckpt


def regressor_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the ``Regressor`` keys out of a ``SegmentSynthesis`` state dict (``regressor.*``, or its duplicate
    ``cfm_wrapper.regressor.*``), or ``sd`` itself when it already is one.  Checks every tensor the decoder reads:
    ``KeyError`` naming a missing one, ``ValueError`` for a foreign shape."""
    reg = _strip(sd, "regressor.")
    if not reg:
        reg = _strip(sd, "cfm_wrapper.regressor.")
    if not reg:
        reg = sd
    for name, shape in regressor_shapes().items():
        if name not in reg:
            raise KeyError("checkpoint is missing regressor tensor %s" % name)
        if tuple(reg[name].shape) != shape:
            raise ValueError("regressor tensor %s has shape %s, expected %s: the HIP decoder is built for the sylber_resynthesis.yaml "
                             "geometry only" % (name, tuple(reg[name].shape), shape))
    return reg


def threshold_from_stats(signal_mean, signal_var, noise_mean, noise_var, eta: float = 1.0) -> float:
    """``Thresholder.get_threshold()`` (sylber/utils/segment_utils.py:27-52) on the host in torch fp32, in the reference's order of
    operations: the crossing point of the two Gaussians N(mu_S, var_S) and N(mu_N, var_N) (+1e-8 on both variances)."""
    f = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(1)       # noqa: E731
    mu_s, mu_n = f(signal_mean), f(noise_mean)
    sd_s, sd_n = (f(signal_var) + 1e-8) ** .5, (f(noise_var) + 1e-8) ** .5
    vs, vn = sd_s ** 2, sd_n ** 2
    qa = vs - vn
    qb = -2 * vs * mu_n + 2 * vn * mu_s
    qc = vs * mu_n ** 2 - vn * mu_s ** 2 - 2 * vn * vs * (np.log(eta) + torch.log(sd_s / sd_n))
    if qa != 0:
        disc = qb ** 2 - 4 * qa * qc
        if disc > 0:
            return float(((-qb + ((mu_s > mu_n) * 1.0) * torch.sqrt(disc)) / (2 * qa)).item())
        if disc == 0:
            return float((-qb / (2 * qa)).item())
        raise ValueError("thresholder statistics have no crossing point (negative discriminant)")
    if qb != 0:
        return float((-qc / qb).item())
    raise ValueError("thresholder statistics are degenerate (equal variances and means)")


def cfm_packed_layout(frames: Sequence[int]) -> np.ndarray:
    """The decoder slots of a packed batch (``sylber_cfm_packed_layout``; host only, no GPU): per-clip frame counts -> int32 ``[B + 1]``
    slot offsets.  Clip b's slot holds ``round_up(16 + frames[b], 64)`` rows: its 16 register rows, its frames and zero rows.
    ValueError for an empty batch, a count below 1 or slots totalling 2^24 rows or more."""
    lib = _lib.load()
    fl = [int(f) for f in frames]
    if not fl:
        raise ValueError("a packed batch needs at least one clip")
    if any(f < 1 or f > 2 ** 31 - 1 for f in fl):
        raise ValueError("every clip of a packed batch needs 1 .. 2^31 - 1 frames, got %s" % fl)
    off = (ctypes.c_int32 * (len(fl) + 1))()
    if lib.sylber_cfm_packed_layout((ctypes.c_int32 * len(fl))(*fl), len(fl), off) != 0:
        raise ValueError(lib.sylber_last_error().decode())
    return np.frombuffer(off, dtype=np.int32).copy()


def _frame_starts(frames: Sequence[int]) -> np.ndarray:
    """[B + 1] prefix sums: clip b's frames are rows [starts[b], starts[b + 1]) of a back-to-back [sum frames, ...] tensor"""
    return np.concatenate([[0], np.cumsum(np.asarray(frames, np.int64))]).astype(np.int64)


def _padded_rows(frames: Sequence[int], T: int, device) -> torch.Tensor:
    """the flat row b * T + t of every clip frame (b, t < frames[b]) of a padded [B, T, ...] tensor, in back-to-back order"""
    idx = np.concatenate([b * T + np.arange(int(f), dtype=np.int64) for b, f in enumerate(frames)])
    return torch.from_numpy(idx).to(device)


def _as_f32(t) -> torch.Tensor:
    return t.detach().to("cpu", torch.float32).contiguous()


class CfmDecoder:
    """The resynthesis decoder behind ``sylber_cfm_*`` (include/sylber_hip.h): ``sample`` = ``cfm_wrapper.sample``,
    ``eval`` = one ``Regressor`` evaluation.  ``state_dict``: ``Regressor.state_dict()`` keys (or a ``SegmentSynthesis``
    dict, see ``regressor_state_dict``)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", precision: str = "bf16"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SylberHipError("no MI355X visible to PyTorch-ROCm; the HIP path has no CPU fallback")
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(PRECISIONS))
        sd = regressor_state_dict(state_dict)
        keep = []

        def ptr(name):
            t = _as_f32(sd[name])
            keep.append(t)
            return ctypes.cast(t.data_ptr(), _lib.c_float_p)

        w = _lib.SylberCfmWeights()
        w.proj_in_w, w.proj_in_b = ptr("proj_in.weight"), ptr("proj_in.bias")
        w.time_freq, w.time_w, w.time_b = ptr("sinu_pos_emb.0.weights"), ptr("sinu_pos_emb.1.weight"), ptr("sinu_pos_emb.1.bias")
        w.to_embed_w, w.to_embed_b = ptr("to_embed.weight"), ptr("to_embed.bias")
        w.conv_w, w.conv_b = ptr("conv_embed.dw_conv1d.0.weight"), ptr("conv_embed.dw_conv1d.0.bias")
        w.register_tokens = ptr("transformer.register_tokens")
        w.rotary_inv_freq = ptr("transformer.rotary_emb.inv_freq")
        for i in range(CFM_DEPTH):
            p = "transformer.layers.%d." % i
            L = w.layers[i]
            L.attn_gamma_w, L.attn_gamma_b = ptr(p + "2.to_gamma.weight"), ptr(p + "2.to_gamma.bias")
            L.attn_beta_w, L.attn_beta_b = ptr(p + "2.to_beta.weight"), ptr(p + "2.to_beta.bias")
            L.q_gamma, L.k_gamma = ptr(p + "3.q_norm.gamma"), ptr(p + "3.k_norm.gamma")
            L.qkv_w, L.out_w = ptr(p + "3.to_qkv.weight"), ptr(p + "3.to_out.weight")
            L.ff_gamma_w, L.ff_gamma_b = ptr(p + "4.to_gamma.weight"), ptr(p + "4.to_gamma.bias")
            L.ff_beta_w, L.ff_beta_b = ptr(p + "4.to_beta.weight"), ptr(p + "4.to_beta.bias")
            L.ff1_w, L.ff1_b = ptr(p + "5.0.weight"), ptr(p + "5.0.bias")
            L.ff2_w, L.ff2_b = ptr(p + "5.3.weight"), ptr(p + "5.3.bias")
        w.final_gamma = ptr("transformer.final_norm.gamma")
        w.to_pred_w = ptr("to_pred.weight")
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.precision = precision
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.sylber_cfm_create(ctypes.byref(w), self.device.index or 0, PRECISIONS[precision], ctypes.byref(self.handle)),
                   "sylber_cfm_create")
        del keep

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.sylber_cfm_destroy(h)
            self.handle = None

    def _cond(self, cond_emb: torch.Tensor) -> torch.Tensor:
        if cond_emb.dim() != 3 or cond_emb.shape[-1] != CFM_DIM_COND_EMB:
            raise ValueError("cond_emb must be [B, T, %d], got %s" % (CFM_DIM_COND_EMB, tuple(cond_emb.shape)))
        if cond_emb.shape[0] < 1 or cond_emb.shape[1] < 1:
            raise ValueError("cond_emb must have B >= 1 and T >= 1, got %s" % (tuple(cond_emb.shape),))
        return cond_emb.to(self.device, torch.float32).contiguous()

    def _state(self, y: Optional[torch.Tensor], cond: torch.Tensor, name: str) -> Optional[torch.Tensor]:
        if y is None:
            return None
        B, T, _ = cond.shape
        if tuple(y.shape) != (B, T, CFM_DIM_OUT):
            raise ValueError("%s must be [%d, %d, %d], got %s" % (name, B, T, CFM_DIM_OUT, tuple(y.shape)))
        return y.to(self.device, torch.float32).contiguous()

    def _workspace(self, B: int, T: int) -> torch.Tensor:
        n = int(self.lib.sylber_cfm_workspace_bytes(self.handle, B, T))
        if n < 0:
            _lib.check(1, "sylber_cfm_workspace_bytes")
        return torch.empty(n, dtype=torch.uint8, device=self.device)

    def _call(self, what: str, fn, args, out, tap: Optional[int], tap_floats):
        """one library call -> ``out``.  ``tap`` (development aid, ``_lib.CFM_TAP_*`` / ``_lib.CFM_TAP(block, k)``, see
        include/sylber_hip_dev.h): set around this one call, which then stops behind the tapped launch of its first evaluation and
        returns that buffer instead -- flat fp32, ``tap_floats()`` values in storage order -- leaving ``out`` unwritten."""
        if tap is None:
            _lib.check(fn(*args), what)
            return out
        n = int(tap_floats())
        if n < 0:
            raise ValueError("%s: no tap stage %r in precision %r" % (what, tap, self.precision))
        buf = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.sylber_cfm_set_tap(self.handle, int(tap), ctypes.c_void_p(buf.data_ptr()), n), "sylber_cfm_set_tap")
        try:
            _lib.check(fn(*args), what)
        finally:
            self.lib.sylber_cfm_set_tap(self.handle, 0, None, 0)
        return buf

    def sample(self, cond_emb: torch.Tensor, steps: int = 5, y0: Optional[torch.Tensor] = None, pitch_amp: float = 1.0,
               frames: Optional[Sequence[int]] = None, tap: Optional[int] = None) -> torch.Tensor:
        """``cfm_wrapper.sample(cond_emb=..., steps=...)`` from ``y0`` (None: zeros, i.e. ``rand_scale = 0``), then channel 12
        divided by ``pitch_amp`` -> ``[B, T, 14]`` fp32 on the device (with ``tap``: the tap's flat fp32 buffer instead).  Enqueued on the current stream.
        ``frames``: each row's own frame count (``sylber_cfm_sample_frames``): row b is sampled as ``cond_emb[b:b+1, :frames[b]]``
        alone would be, and ``art[b, frames[b]:]`` is 0.  Counts outside ``[1, T]`` raise ValueError.  ``tap``: see ``_call``."""
        if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= 65:
            raise ValueError("steps must be an integer in 1..65, got %r" % (steps,))
        cond = self._cond(cond_emb)
        y0 = self._state(y0, cond, "y0")
        B, T, _ = cond.shape
        farr = None
        if frames is not None:
            fl = [int(f) for f in frames]
            if len(fl) != B or any(f < 1 or f > T for f in fl):
                raise ValueError("frames must hold %d counts in [1, %d], got %s" % (B, T, fl))
            farr = (ctypes.c_int32 * B)(*fl)
        art = torch.empty(B, T, CFM_DIM_OUT, dtype=torch.float32, device=self.device)
        ws = self._workspace(B, T)
        tail = (int(steps), ctypes.c_void_p(y0.data_ptr()) if y0 is not None else None, ctypes.c_float(float(pitch_amp)),
                ctypes.c_void_p(art.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        with torch.cuda.device(self.device):
            if farr is None:
                return self._call("sylber_cfm_sample", self.lib.sylber_cfm_sample, (self.handle, ctypes.c_void_p(cond.data_ptr()), B, T) + tail,
                                  art, tap, lambda: self.lib.sylber_cfm_tap_floats(self.handle, int(tap), B, T))
            return self._call("sylber_cfm_sample_frames", self.lib.sylber_cfm_sample_frames,
                              (self.handle, ctypes.c_void_p(cond.data_ptr()), farr, B, T) + tail, art, tap,
                              lambda: self.lib.sylber_cfm_tap_floats(self.handle, int(tap), B, T))

    def sample_packed(self, conds, steps: int = 5, y0: Optional[torch.Tensor] = None, pitch_amp: float = 1.0, tap: Optional[int] = None):
        """A ragged batch without padding to its longest clip (``sylber_cfm_sample_packed``, bf16 / fp16).  ``conds``: a list of
        ``[T_b, 256]`` tensors, or ``(packed [sum T_b, 256], frames)``.  ``y0``: ``[sum T_b, 14]`` in the same order, or None (zeros).
        Returns ``(art [sum T_b, 14] fp32 on the device, starts)``: clip b is ``art[starts[b]:starts[b + 1]]``, bit-identical to
        ``sample(cond, frames=...)``'s row b and to the clip sampled alone.  ValueError before any launch for an fp32 decoder, bad counts
        or shapes.  ``tap`` (see ``_call``): returns ``(the tap's buffer, starts)``."""
        if self.precision not in PACKED_PRECISIONS:
            raise ValueError("sample_packed: packed batches run in precision %s only (this decoder: %r)"
                             % (" / ".join(map(repr, PACKED_PRECISIONS)), self.precision))
        if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= 65:
            raise ValueError("steps must be an integer in 1..65, got %r" % (steps,))
        if isinstance(conds, tuple) and len(conds) == 2 and torch.is_tensor(conds[0]):
            cond, frames = conds
            fl = [int(f) for f in frames]
        else:
            parts = list(conds)
            if not parts:
                raise ValueError("a packed batch needs at least one clip")
            for c in parts:
                if c.dim() != 2 or c.shape[-1] != CFM_DIM_COND_EMB:
                    raise ValueError("each clip's cond must be [T_b, %d], got %s" % (CFM_DIM_COND_EMB, tuple(c.shape)))
            fl = [int(c.shape[0]) for c in parts]
            cond = torch.cat([c.to(self.device, torch.float32) for c in parts]) if all(f > 0 for f in fl) else None
        if not fl or any(f < 1 for f in fl):
            raise ValueError("every clip needs >= 1 frame, got %s" % fl)
        B, NF = len(fl), sum(fl)
        if cond is None or cond.dim() != 2 or tuple(cond.shape) != (NF, CFM_DIM_COND_EMB):
            raise ValueError("packed cond must be [sum T_b = %d, %d], got %s" % (NF, CFM_DIM_COND_EMB, None if cond is None else tuple(cond.shape)))
        cond = cond.to(self.device, torch.float32).contiguous()
        if y0 is not None:
            if tuple(y0.shape) != (NF, CFM_DIM_OUT):
                raise ValueError("y0 must be [%d, %d], got %s" % (NF, CFM_DIM_OUT, tuple(y0.shape)))
            y0 = y0.to(self.device, torch.float32).contiguous()
        farr = (ctypes.c_int32 * B)(*fl)
        n = int(self.lib.sylber_cfm_workspace_bytes_packed(self.handle, farr, B))
        if n < 0:
            raise ValueError(self.lib.sylber_last_error().decode())
        ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        art = torch.empty(NF, CFM_DIM_OUT, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            art = self._call("sylber_cfm_sample_packed", self.lib.sylber_cfm_sample_packed,
                             (self.handle, ctypes.c_void_p(cond.data_ptr()), farr, B, int(steps),
                              ctypes.c_void_p(y0.data_ptr()) if y0 is not None else None, ctypes.c_float(float(pitch_amp)),
                              ctypes.c_void_p(art.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                              ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                             art, tap, lambda: self.lib.sylber_cfm_tap_floats_packed(self.handle, int(tap), farr, B))
        return art, _frame_starts(fl)

    def eval(self, x: torch.Tensor, t: float, cond_emb: torch.Tensor, tap: Optional[int] = None) -> torch.Tensor:
        """one velocity evaluation of the ``Regressor`` at state ``x [B, T, 14]`` and time ``t`` -> ``[B, T, 14]`` fp32 on the device
        (with ``tap``, see ``_call``: the tap's flat fp32 buffer instead)."""
        cond = self._cond(cond_emb)
        x = self._state(x, cond, "x")
        B, T, _ = cond.shape
        v = torch.empty(B, T, CFM_DIM_OUT, dtype=torch.float32, device=self.device)
        ws = self._workspace(B, T)
        with torch.cuda.device(self.device):
            return self._call("sylber_cfm_eval", self.lib.sylber_cfm_eval,
                              (self.handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_float(float(t)), ctypes.c_void_p(cond.data_ptr()), B, T,
                               ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                               ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), v, tap,
                              lambda: self.lib.sylber_cfm_tap_floats(self.handle, int(tap), B, T))


class SegmentSynthesis:
    """Same constructor and ``resynthesize`` contract as the reference's ``SegmentSynthesis``
    (sylber/model/segment_synthesis.py:57-146), inference only.  ``model_ckpt``: a path or a state dict with the keys of
    ``SegmentSynthesis.state_dict()`` (``speech_model.*``, ``input_model.mlp.*``, ``regressor.*`` / ``cfm_wrapper.regressor.*``,
    ``thresholder.*``), optionally inside a Lightning ``{"state_dict": {"net.<key>": ...}}`` wrapper.  ``precision``:
    "bf16" (default), "fp16" or "fp32" (parity mode), for the encoder and the decoder alike.
    ``quantizer``: None, a ``KMQuantizer`` / ``ResidualKMQuantizer``, a learned ``Quantizer`` (``tokenize`` only: its decode is
    not a feature row, so ``resynthesize`` / ``synthesize_units`` refuse it), or a ``.npy`` codebook path; with a path,
    ``residual_quantizer`` (a second ``.npy`` path) makes it a ``ResidualKMQuantizer`` and ``normalize_embed`` is the
    ``KMQuantizer``'s ``normalize`` (what upstream's constructor, segment_synthesis.py:93-99, means to do).
    ``packed=True`` (bf16 / fp16): ragged batches run without padding to the longest clip in the encoder, the conditioning and the
    decoder, with ``batch_invariant=True``'s results bit for bit (it implies that mode)."""

    def __init__(self, model_ckpt=None, speech_upstream="facebook/hubert-base-ls960", encoding_layer=9, input_configs=None,
                 regressor_configs=None, thresholder_configs=None, pitch_amp=5, quantizer=None, device="cuda", precision="bf16",
                 **kwargs):
        if "cuda" not in str(device):
            raise _lib.SylberHipError("sylber_amd.SegmentSynthesis runs on the MI355X only (device=%r)" % (device,))
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(PRECISIONS))
        self.packed = bool(kwargs.get("packed", False))
        if self.packed and precision not in PACKED_PRECISIONS:
            raise ValueError("packed=True supports precision %s only (got %r)" % (" / ".join(map(repr, PACKED_PRECISIONS)), precision))
        self.input_configs = dict(DEFAULT_INPUT_CONFIGS if input_configs is None else input_configs)
        self.regressor_configs = dict(DEFAULT_REGRESSOR_CONFIGS if regressor_configs is None else regressor_configs)
        self.thresholder_configs = dict(DEFAULT_THRESHOLDER_CONFIGS if thresholder_configs is None else thresholder_configs)
        check_regressor_configs(self.regressor_configs)
        if int(self.input_configs.get("output_dim", CFM_DIM_COND_EMB)) != CFM_DIM_COND_EMB:
            raise ValueError("input_configs['output_dim'] must equal the decoder's dim_cond_emb (%d)" % CFM_DIM_COND_EMB)
        if model_ckpt is None:
            raise ValueError("model_ckpt is required (a path or a SegmentSynthesis state dict)")
        sd = unwrap_checkpoint(model_ckpt)
        self.pitch_amp = pitch_amp
        self.encoding_layer = encoding_layer
        self.speech_upstream = speech_upstream
        speech = _strip(sd, "speech_model.")
        if not speech:
            raise KeyError("checkpoint is missing the speech_model.* tensors")
        mlp = _strip(sd, "input_model.")
        if not mlp:
            raise KeyError("checkpoint is missing the input_model.* tensors")
        self.decoder = CfmDecoder(sd, device=device, precision=precision)     # checks the regressor tensors first (cheapest to fail)
        self.speech_model = HubertEncoderHIP(speech, num_layers=encoding_layer, device=device, precision=precision)
        # batch-invariant mode (off by default): each row of a padded batch is resynthesized exactly as it is alone
        # packed batches (off by default) keep batch-invariant mode's results, so they imply it
        self.batch_invariant = bool(kwargs.get("batch_invariant", False)) or self.packed
        if self.batch_invariant:
            self.speech_model.set_per_utterance(True)
        self.input_model = SegmentConditioner(mlp, device=device)
        self.device = self.speech_model.device
        residual = kwargs.get("residual_quantizer")
        if isinstance(quantizer, (str, Path)):
            if residual is not None:
                quantizer = ResidualKMQuantizer(str(quantizer), str(residual), device=self.device)
            else:
                quantizer = KMQuantizer(str(quantizer), normalize=bool(kwargs.get("normalize_embed", False)), device=self.device)
        elif residual is not None:
            raise ValueError("residual_quantizer is a codebook path that goes with a quantizer path; pass a ResidualKMQuantizer instead")
        self.quantizer = quantizer                     # KMQuantizer / ResidualKMQuantizer (or None), passed to SegmentConditioner
        thr = _strip(sd, "thresholder.")
        if "threshold" in thr:
            self._threshold = float(thr["threshold"].reshape(-1)[0])
        elif all(k in thr for k in ("signal_mean", "signal_var", "noise_mean", "noise_var")):
            self._threshold = threshold_from_stats(thr["signal_mean"], thr["signal_var"], thr["noise_mean"], thr["noise_var"])
        else:
            c = self.thresholder_configs
            self._threshold = threshold_from_stats(c["signal_mean"], c["signal_var"], c["noise_mean"], c["noise_var"])

    def get_threshold(self) -> float:
        """``thresholder.get_threshold()``: the checkpoint's thresholder statistics, else ``thresholder_configs``'"""
        return self._threshold

    def resynthesize(self, input_values=None, attention_mask=None, features=None, steps=5, rand_scale=0.0, merge_threshold=0.8,
                     normthreshold=None, prosody_steps=None, prosody_rand_scale=None, y0=None, frames=None):
        """-> ``(art [B, T, 14] fp32 on the device, segments)`` with channel 12 divided by ``pitch_amp``; ``segments`` is a list of
        int64 ``[n, 2]`` arrays (``np.array([])`` for none), or None on the ``features=`` branch.  ``rand_scale > 0`` starts the
        sampler from ``randn_like(cond) * rand_scale`` on the device; ``y0=`` supplies that start explicitly (tests).
        ``prosody_*`` are accepted and ignored, as upstream.
        With ``batch_invariant=True``, row b of ``art[:, :T_b]`` (``T_b`` from ``attention_mask``) and its segments are bit-identical
        to the clip resynthesized alone, and ``art[b, T_b:]`` is 0.  ``frames=`` gives the ``features=`` branch each row's frame count
        (default: every row ``T`` frames).
        With ``packed=True`` the results are batch-invariant mode's, bit for bit; ``input_values`` may also be a list of 1-D clips (then
        ``T`` is the longest clip's frame count)."""
        dev = self.device
        if self.packed:
            return self._resynthesize_packed(input_values, attention_mask, features, steps, rand_scale, merge_threshold, normthreshold, y0,
                                             frames)
        if features is None:
            if input_values is None:
                raise ValueError("pass input_values or features")
            if isinstance(self.quantizer, Quantizer):
                raise ValueError(LEARNED_QUANTIZER_NO_FEATURES)
            if normthreshold is None:
                normthreshold = self.get_threshold()
            hidden, frames, seg, nseg, feats, nseg_h, seg_h = self.speech_model.segment_batch(input_values, attention_mask, normthreshold,
                                                                                              merge_threshold, self.batch_invariant)
            if not self.batch_invariant:
                frames = None
            cond, _ = self.input_model(hidden, seg, nseg, feats, normthreshold, quantizer=self.quantizer)
            segments = _segment_list(seg_h, nseg_h)
        else:
            feats = torch.as_tensor(features).to(dev, torch.float32).contiguous()
            if feats.dim() != 3:
                raise ValueError("features must be [B, T, 768]")
            cond = self.input_model.from_features(feats)
            segments = None
        if y0 is None and rand_scale:
            y0 = torch.randn(cond.shape[0], cond.shape[1], CFM_DIM_OUT, device=dev) * rand_scale
        art = self.decoder.sample(cond, steps=steps, y0=y0, pitch_amp=self.pitch_amp, frames=frames)
        return art, segments

    # ---- packed batches ----------------------------------------------------------------------------------------------------
    def _clips(self, input_values, attention_mask):
        """-> (1-D clips, T of the padded result or None): a list of clips, one clip, or a padded [B, N] batch cut by its mask"""
        if isinstance(input_values, (list, tuple)):
            if attention_mask is not None:
                raise ValueError("a list of clips carries its own lengths; do not pass attention_mask")
            clips = [torch.as_tensor(c).reshape(-1) for c in input_values]
            if not clips:
                raise ValueError("a packed batch needs at least one clip")
            return clips, None
        x = torch.as_tensor(input_values)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError("input_values must be [B, N], [N] or a list of 1-D clips")
        B, N = x.shape
        lengths = [N] * B if attention_mask is None else [int(v) for v in torch.as_tensor(attention_mask).sum(-1).reshape(-1).tolist()]
        if len(lengths) != B:
            raise ValueError("attention_mask must have one row per clip")
        return [x[b, :lengths[b]] for b in range(B)], self.speech_model.num_frames(N)

    def _encode_packed(self, input_values, attention_mask, normthreshold, merge_threshold):
        """encoder and boundary detection of a packed batch -> (hidden, offsets, frames, seg, nseg, feats, nseg_h, seg_h, T)"""
        sm = self.speech_model
        sm._check_packed("SegmentSynthesis(packed=True)")
        clips, T = self._clips(input_values, attention_mask)
        hidden, offsets, frames = sm.forward_packed(clips)
        lengths = [int(c.numel()) for c in clips]
        seg, nseg, feats = sm.segment_packed(hidden, lengths, normthreshold, merge_threshold, layout=(offsets, frames))
        nseg_h, seg_h = _tables_to_host(seg, nseg)
        return hidden, offsets, frames, seg, nseg, feats, nseg_h, seg_h, (T if T is not None else int(frames.max()))

    def _sample_packed(self, cond: torch.Tensor, frames, T: int, steps, rand_scale, y0) -> torch.Tensor:
        """the decoder over each clip's own frames (cond [sum frames, 256]) -> padded art [B, T, 14], zeros past each clip's frames.
        rand_scale / a padded y0 [B, T, 14]: the batch-invariant call's start state, each clip's rows taken from it."""
        dev = self.device
        fl = [int(f) for f in frames]
        B = len(fl)
        idx = _padded_rows(fl, T, dev)
        if y0 is None and rand_scale:
            y0 = torch.randn(B, T, CFM_DIM_OUT, device=dev) * rand_scale
        if y0 is not None:
            y0 = torch.as_tensor(y0).to(dev, torch.float32)
            if tuple(y0.shape) != (B, T, CFM_DIM_OUT):
                raise ValueError("y0 must be [%d, %d, %d], got %s" % (B, T, CFM_DIM_OUT, tuple(y0.shape)))
            y0 = y0.reshape(B * T, CFM_DIM_OUT).index_select(0, idx)
        art_p, _ = self.decoder.sample_packed((cond, fl), steps=steps, y0=y0, pitch_amp=self.pitch_amp)
        art = torch.zeros(B, T, CFM_DIM_OUT, dtype=torch.float32, device=dev)
        art.view(B * T, CFM_DIM_OUT).index_copy_(0, idx, art_p)
        return art

    def _resynthesize_packed(self, input_values, attention_mask, features, steps, rand_scale, merge_threshold, normthreshold, y0, frames):
        dev = self.device
        if features is None:
            if input_values is None:
                raise ValueError("pass input_values or features")
            if isinstance(self.quantizer, Quantizer):
                raise ValueError(LEARNED_QUANTIZER_NO_FEATURES)
            if normthreshold is None:
                normthreshold = self.get_threshold()
            hidden, offsets, fr, seg, nseg, feats, nseg_h, seg_h, T = self._encode_packed(input_values, attention_mask, normthreshold,
                                                                                          merge_threshold)
            cond = self.input_model.packed(hidden, offsets, fr, seg, nseg, feats, normthreshold, quantizer=self.quantizer)
            return self._sample_packed(cond, fr, T, steps, rand_scale, y0), _segment_list(seg_h, nseg_h)
        feats = torch.as_tensor(features).to(dev, torch.float32).contiguous()
        if feats.dim() != 3:
            raise ValueError("features must be [B, T, 768]")
        B, T, D = feats.shape
        fl = [T] * B if frames is None else [int(f) for f in frames]
        if len(fl) != B or any(f < 1 or f > T for f in fl):
            raise ValueError("frames must hold %d counts in [1, %d], got %s" % (B, T, fl))
        if D != self.input_model.input_dim:
            raise ValueError("feature dim %d != MLP input dim %d" % (D, self.input_model.input_dim))
        rows = feats.reshape(B * T, D).index_select(0, _padded_rows(fl, T, dev))
        cond = self.input_model.from_features(rows)
        return self._sample_packed(cond, fl, T, steps, rand_scale, y0), None

    def tokenize(self, input_values, attention_mask=None, merge_threshold=0.8, normthreshold=None) -> List[dict]:
        """speech -> syllable units: one dict per clip with ``units`` int64 ``[n, ncb]`` (the quantizer's ids of the clip's segment
        means: ncb = 1 for a ``KMQuantizer``, 2 for a ``ResidualKMQuantizer``, Qa + Qp for a learned ``Quantizer``), ``segments`` int64 ``[n, 2]`` (the table
        ``resynthesize`` returns; ``[0, 2]`` for none) and ``frames`` (the clip's own frame count).  Everything up to the ids runs on the
        device; slots past a clip's segment count are zeroed there.  ``synthesize_units(tokenize(wav))`` is bitwise
        ``resynthesize(wav)`` with ``batch_invariant=True``.  ``ValueError`` without a quantizer."""
        if self.quantizer is None:
            raise ValueError("tokenize needs a quantizer (SegmentSynthesis(quantizer=...))")
        dev = self.device
        if normthreshold is None:
            normthreshold = self.get_threshold()
        if self.packed:
            _, _, frames, _, nseg, feats, nseg_h, seg_h, _ = self._encode_packed(input_values, attention_mask, normthreshold, merge_threshold)
        else:
            _, frames, _, nseg, feats, nseg_h, seg_h = self.speech_model.segment_batch(input_values, attention_mask, normthreshold,
                                                                                       merge_threshold, self.batch_invariant)
        S = seg_h.shape[1]
        keep = torch.arange(S, device=dev)[None, :] < nseg[:, None].to(torch.int64)
        head = torch.where(keep[:, :, None], feats[:, :S], torch.zeros((), device=dev)).contiguous()
        ids = self.quantizer.get_indices(head).cpu().numpy()
        return [{"units": ids[b, :int(n)].astype(np.int64), "segments": seg_h[b, :int(n)].astype(np.int64).reshape(-1, 2),
                 "frames": int(frames[b])} for b, n in enumerate(nseg_h)]

    def synthesize_units(self, units, segments=None, frames=None, steps=5, rand_scale=0.0, y0=None, nunits=None) -> torch.Tensor:
        """syllable units -> ``art [B, T, 14]`` fp32 on the device (channel 12 divided by ``pitch_amp``): each unit's decoded codebook
        row (the sum of the quantizer's codebooks) conditions the frames of its segment, frames outside every segment and units whose
        decoded row has norm < 1e-4 get a zero conditioning row, and the decoder samples row b over its own ``frames[b]`` frames
        (``art[b, frames[b]:]`` is 0, as in batch-invariant mode).  ``T = max(frames)``.
        Bitwise ``resynthesize(features=expand_feature(decode(units), durations), frames=frames)``, with the conditioning MLP run once
        per unit instead of once per frame.
        ``units``: the list ``tokenize`` returns; or a list of per-clip int arrays ``[n_b, ncb]`` with ``segments`` a list of ``[n_b, 2]``
        frame spans; or a padded ``[B, S, ncb]`` tensor with ``segments [B, S, 2]`` and ``nunits [B]``.  ``frames`` defaults to each
        clip's last segment end (1 for a clip without units)."""
        if self.quantizer is None:
            raise ValueError("synthesize_units needs a quantizer (SegmentSynthesis(quantizer=...))")
        if isinstance(self.quantizer, Quantizer):
            raise ValueError(LEARNED_QUANTIZER_NO_FEATURES)
        books = quantizer_codebooks(self.quantizer)
        ncb = len(books)
        if isinstance(units, (list, tuple)):
            if units and isinstance(units[0], dict):
                if segments is not None:
                    raise ValueError("segments come with tokenize()'s dicts; do not pass them again")
                if frames is None:
                    frames = [int(u["frames"]) for u in units]
                units, segments = [u["units"] for u in units], [u["segments"] for u in units]
            if segments is None or len(segments) != len(units) or not units:
                raise ValueError("pass one segment table per clip")
            ul = [np.asarray(u.cpu() if torch.is_tensor(u) else u, dtype=np.int64) for u in units]
            for u in ul:
                if not (u.ndim == 2 and u.shape[-1] == ncb) and not (u.ndim == 1 and ncb == 1):
                    raise ValueError("this quantizer decodes %d id(s) per unit: units must be [n, %d], got %s" % (ncb, ncb, u.shape))
            ul = [u.reshape(-1, ncb) for u in ul]
            sl = [np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.int64).reshape(-1, 2) for s in segments]
            if any(len(u) != len(s) for u, s in zip(ul, sl)):
                raise ValueError("each clip needs one segment per unit, got %s units and %s segments"
                                 % ([len(u) for u in ul], [len(s) for s in sl]))
            B, S = len(ul), max(1, max(len(u) for u in ul))
            U = np.zeros((B, S, ncb), np.int64)
            P = np.zeros((B, S, 2), np.int64)
            for b, (u, s) in enumerate(zip(ul, sl)):
                U[b, :len(u)], P[b, :len(s)] = u, s
            counts = [len(u) for u in ul]
        else:
            if segments is None or nunits is None:
                raise ValueError("a padded units tensor needs segments [B, S, 2] and nunits [B]")
            U = torch.as_tensor(units).cpu().numpy().astype(np.int64)
            P = torch.as_tensor(segments).cpu().numpy().astype(np.int64)
            counts = [int(n) for n in torch.as_tensor(nunits).reshape(-1).tolist()]
            if U.ndim != 3 or U.shape[-1] != ncb or P.shape != U.shape[:2] + (2,) or len(counts) != U.shape[0]:
                raise ValueError("units [B, S, %d], segments [B, S, 2] and nunits [B] expected, got %s, %s, %d counts"
                                 % (ncb, U.shape, P.shape, len(counts)))
            B, S = U.shape[0], max(U.shape[1], 1)
        if U.shape[-1] != ncb:
            raise ValueError("this quantizer decodes %d id(s) per unit, got %d" % (ncb, U.shape[-1]))
        if frames is None:
            frames = [int(P[b, counts[b] - 1, 1]) if 0 < counts[b] <= P.shape[1] else 1 for b in range(B)]
        frames = [int(f) for f in frames]
        if len(frames) != B or min(frames) < 1:
            raise ValueError("frames must hold %d counts >= 1, got %s" % (B, frames))
        T = max(frames)
        for arr, name in ((U, "unit ids"), (P, "spans")):
            if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
                raise ValueError("%s do not fit int32" % name)
        dev = self.device
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).to(dev)   # noqa: E731
        if U.shape[1] == 0:
            U, P = np.zeros((B, 1, ncb), np.int64), np.zeros((B, 1, 2), np.int64)
        if self.packed:
            cond = self.input_model.from_units(books, i32(U), i32(P), i32(counts), None, frames=i32(frames))
            return self._sample_packed(cond, frames, T, steps, rand_scale, y0)
        cond = self.input_model.from_units(books, i32(U), i32(P), i32(counts), T, frames=i32(frames))
        if y0 is None and rand_scale:
            y0 = torch.randn(cond.shape[0], cond.shape[1], CFM_DIM_OUT, device=dev) * rand_scale
        return self.decoder.sample(cond, steps=steps, y0=y0, pitch_amp=self.pitch_amp, frames=frames)
