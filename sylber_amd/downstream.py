"""Host mirrors of the two callers right behind the Segmenter path, running on the
device-resident outputs of ``HubertEncoderHIP.segment`` through the C-ABI (csrc/downstream.hip):

* ``KMQuantizer`` — sylber/model/quantizer.py:86-135: ``get_indices`` (nearest centroid) and ``decode``;
* ``ResidualKMQuantizer`` — quantizer.py:137-180: two-stage k-means, ``indices [..., 2]``, ``decode`` = ``z_q1 + z_q2``;
* ``expand_feature`` — sylber/model/flowmatching.py:873-882: unit features laid out over frames by ``durations``;
* ``SegmentConditioner`` — the front half of ``SegmentSynthesis.resynthesize`` (sylber/model/segment_synthesis.py:
  103-140): segment means broadcast back to frames -> ``MLP`` conditioner -> silence mask."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib


def _vp(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class KMQuantizer:
    """``KMQuantizer(centroids, normalize=False)`` — ``centroids`` a ``.npy`` path (like the reference) or an
    array/tensor ``[K, 768]``."""

    def __init__(self, centroids, normalize: bool = False, device="cuda"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SylberHipError("no MI355X visible to PyTorch-ROCm; the HIP path has no CPU fallback")
        if isinstance(centroids, str):
            centroids = np.load(centroids)
        c = torch.as_tensor(np.asarray(centroids) if not torch.is_tensor(centroids) else centroids, dtype=torch.float32)
        if c.dim() != 2:
            raise ValueError("centroids must be [K, D]")
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.centroids = c.contiguous().to(self.device)
        self.normalize = normalize

    def get_indices(self, token: torch.Tensor) -> torch.Tensor:
        """token ``[..., D]`` -> int64 indices ``[..., 1]`` (the reference's ``outputs['indices']`` for one codebook)"""
        lead = tuple(token.shape[:-1])
        x = token.reshape(-1, token.shape[-1]).to(self.device, torch.float32).contiguous()
        n, D = x.shape
        K = self.centroids.shape[0]
        idx = torch.empty(n, dtype=torch.int32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_km_workspace_floats(n, K, D)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_km_assign(_vp(x), n, _vp(self.centroids), K, D, 1 if self.normalize else 0, _vp(idx), _vp(ws),
                                                 _stream(self.device)), "sylber_km_assign")
        return idx.to(torch.int64).reshape(lead + (1,))

    def decode(self, indices: torch.Tensor) -> torch.Tensor:
        """indices ``[..., >=1]`` -> centroid rows ``[..., D]`` (negative indices clipped to 0, quantizer.py:129-130)"""
        ind = indices[..., :1]
        lead = tuple(ind.shape[:-1])
        flat = ind.reshape(-1).to(self.device, torch.int32).contiguous()
        K, D = self.centroids.shape
        out = torch.empty(flat.numel(), D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_km_decode(_vp(flat), flat.numel(), _vp(self.centroids), K, D, _vp(out), _stream(self.device)),
                       "sylber_km_decode")
        return out.reshape(lead + (D,))

    def __call__(self, token: torch.Tensor) -> Dict[str, torch.Tensor]:
        idx = self.get_indices(token)
        return {"indices": idx, "quantize": self.decode(idx), "non_quantized": token}


class ResidualKMQuantizer:
    """``ResidualKMQuantizer(centroids, centroids2, normalize=False)`` (quantizer.py:137-180): stage 1 assigns the token against
    ``centroids``, stage 2 assigns ``token - decode(stage 1)`` against ``centroids2``; ``indices`` are ``[..., 2]`` and ``decode``
    returns ``z_q1 + z_q2``.  ``normalize`` is accepted and ignored, as upstream (whose constructor builds both stages as
    ``KMQuantizer(c)`` without it).  ``centroids`` / ``centroids2``: ``.npy`` paths or arrays / tensors ``[K, 768]``."""

    def __init__(self, centroids, centroids2, normalize: bool = False, device="cuda"):
        self.km = KMQuantizer(centroids, device=device)
        self.km2 = KMQuantizer(centroids2, device=device)
        if self.km.centroids.shape[1] != self.km2.centroids.shape[1]:
            raise ValueError("the two codebooks must have the same width")
        self.lib, self.device = self.km.lib, self.km.device
        self.normalize = normalize

    @property
    def codebooks(self):
        return (self.km.centroids, self.km2.centroids)

    def get_indices(self, token: torch.Tensor) -> torch.Tensor:
        """token ``[..., D]`` -> int64 indices ``[..., 2]`` (stage-1 id, stage-2 id of the residual)"""
        lead = tuple(token.shape[:-1])
        x = token.reshape(-1, token.shape[-1]).to(self.device, torch.float32).contiguous()
        n, D = x.shape
        (c1, c2), K1, K2 = self.codebooks, self.km.centroids.shape[0], self.km2.centroids.shape[0]
        idx = torch.empty(n, 2, dtype=torch.int32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_km_residual_workspace_floats(n, K1, K2, D)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_km_assign_residual(_vp(x), n, _vp(c1), K1, _vp(c2), K2, D, _vp(idx), _vp(ws), _stream(self.device)),
                       "sylber_km_assign_residual")
        return idx.to(torch.int64).reshape(lead + (2,))

    def decode(self, indices: torch.Tensor) -> torch.Tensor:
        """indices ``[..., 2]`` -> ``c1[i1] + c2[i2]`` ``[..., D]`` (negative indices clipped to 0)"""
        if indices.shape[-1] != 2:
            raise ValueError("ResidualKMQuantizer.decode takes indices [..., 2], got %s" % (tuple(indices.shape),))
        lead = tuple(indices.shape[:-1])
        flat = indices.reshape(-1, 2).to(self.device, torch.int32).contiguous()
        (c1, c2), K1, K2 = self.codebooks, self.km.centroids.shape[0], self.km2.centroids.shape[0]
        D = c1.shape[1]
        out = torch.empty(flat.shape[0], D, dtype=torch.float32, device=self.device)
        if flat.shape[0]:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.sylber_km_decode_residual(_vp(flat), flat.shape[0], _vp(c1), K1, _vp(c2), K2, D, _vp(out),
                                                              _stream(self.device)), "sylber_km_decode_residual")
        return out.reshape(lead + (D,))

    def __call__(self, token: torch.Tensor) -> Dict[str, torch.Tensor]:
        idx = self.get_indices(token)
        return {"indices": idx, "quantize": self.decode(idx), "non_quantized": token}


def load_km_quantizer(centroids, normalize: bool = False, device="cuda") -> KMQuantizer:
    """quantizer.py:79-80"""
    return KMQuantizer(centroids, normalize=normalize, device=device)


def load_residualkm_quantizer(centroids, centroids2, normalize: bool = False, device="cuda") -> ResidualKMQuantizer:
    """quantizer.py:82-83 (``normalize`` is ignored there too)"""
    return ResidualKMQuantizer(centroids, centroids2, normalize=normalize, device=device)


LEARNED_QUANTIZER_NO_FEATURES = (
    "a learned Quantizer decodes to its [..., output_dim] art / pitch embedding, not to the 768-d segment feature the conditioning "
    "MLP reads; it can tokenize, but not condition resynthesis (use a KMQuantizer / ResidualKMQuantizer for that)")


def quantizer_codebooks(quantizer) -> Sequence[torch.Tensor]:
    """the codebooks whose rows ``quantizer.decode`` sums: one for a ``KMQuantizer``, two for a ``ResidualKMQuantizer``.  A learned
    ``Quantizer`` is refused: its decode is an art / pitch embedding of ``output_dim`` columns, not a 768-d feature row."""
    from .quantizer import Quantizer
    if isinstance(quantizer, Quantizer):
        raise ValueError(LEARNED_QUANTIZER_NO_FEATURES)
    books = getattr(quantizer, "codebooks", None)
    if books is None:
        books = (quantizer.centroids,)
    return tuple(books)


def expand_feature(avg_fts: torch.Tensor, durations) -> torch.Tensor:
    """``expand_feature(avg_fts, durations)`` (flowmatching.py:873-882) on the device: ``avg_fts [B, S, D]``, ``durations
    [B, S, 2]`` = (frames of the unit, zero frames after it) -> ``[B, T, D]``, every row laid out as
    ``[feat_0] * d00 + [0] * d01 + [feat_1] * d10 + ...``.  Rows whose durations do not sum to the same T raise ValueError
    (upstream's ``torch.stack`` refuses them too)."""
    lib = _lib.load()
    x = torch.as_tensor(avg_fts)
    dev = x.device if x.is_cuda else torch.device("cuda:%d" % torch.cuda.current_device())
    x = x.to(dev, torch.float32).contiguous()
    d = torch.as_tensor(durations)
    if x.dim() != 3 or tuple(d.shape) != (x.shape[0], x.shape[1], 2):
        raise ValueError("expand_feature takes avg_fts [B, S, D] and durations [B, S, 2], got %s and %s"
                         % (tuple(x.shape), tuple(d.shape)))
    dh = d.detach().to("cpu", torch.int64)
    if (dh < 0).any():
        raise ValueError("durations must be >= 0")
    sums = dh.sum(dim=(1, 2)).tolist()
    if len(set(sums)) != 1 or sums[0] < 1:
        raise ValueError("every row's durations must sum to the same T >= 1, got %s" % sums)
    B, S, D = x.shape
    T = int(sums[0])
    out = torch.empty(B, T, D, dtype=torch.float32, device=dev)
    dd = dh.to(torch.int32).to(dev).contiguous()
    ws = torch.empty(B * S + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_expand_units(_vp(x), _vp(dd), B, S, D, T, _vp(out), _vp(ws), _stream(dev)), "sylber_expand_units")
    return out


class SegmentConditioner:
    """``MLP(input_dim, output_dim, hidden_dims)`` of segment_synthesis.py:35-53 + the frame broadcast / silence mask
    of ``resynthesize``.  ``state_dict`` uses the keys of the reference module (``mlp.0.weight`` ...; an
    ``input_model.`` prefix, as in a SegmentSynthesis checkpoint, is accepted)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SylberHipError("no MI355X visible to PyTorch-ROCm; the HIP path has no CPU fallback")
        sd = {(k[len("input_model."):] if k.startswith("input_model.") else k): v for k, v in state_dict.items()}
        lin = sorted({int(k.split(".")[1]) for k in sd if k.startswith("mlp.") and k.count(".") == 2})
        if not lin or lin != list(range(0, 2 * (len(lin) - 1) + 1, 2)):
            raise KeyError("state_dict does not look like MLP.state_dict(): %s" % sorted(sd)[:4])
        nh = len(lin) - 1
        keep = []

        def ptr(name):
            t = sd[name].detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            return ctypes.cast(t.data_ptr(), _lib.c_float_p)

        w = _lib.SylberMlpWeights()
        w.input_dim = int(sd["mlp.0.weight"].shape[1]); w.output_dim = int(sd["mlp.%d.weight" % (2 * nh)].shape[0]); w.num_hidden = nh
        for i in range(nh):
            w.hidden_dims[i] = int(sd["mlp.%d.weight" % (2 * i)].shape[0])
            h = w.hidden[i]
            h.lin_w = ptr("mlp.%d.weight" % (2 * i)); h.lin_b = ptr("mlp.%d.bias" % (2 * i))
            h.ff1_w = ptr("mlp.%d.linear1.weight" % (2 * i + 1)); h.ff1_b = ptr("mlp.%d.linear1.bias" % (2 * i + 1))
            h.ff2_w = ptr("mlp.%d.linear2.weight" % (2 * i + 1)); h.ff2_b = ptr("mlp.%d.linear2.bias" % (2 * i + 1))
            h.ln_w = ptr("mlp.%d.norm.weight" % (2 * i + 1)); h.ln_b = ptr("mlp.%d.norm.bias" % (2 * i + 1))
        w.out_w = ptr("mlp.%d.weight" % (2 * nh)); w.out_b = ptr("mlp.%d.bias" % (2 * nh))
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.input_dim, self.output_dim = w.input_dim, w.output_dim
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.sylber_mlp_create(ctypes.byref(w), self.device.index or 0, ctypes.byref(self.handle)), "sylber_mlp_create")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.sylber_mlp_destroy(h)
            self.handle = None

    def __call__(self, hidden: torch.Tensor, seg: torch.Tensor, nseg: torch.Tensor, feats: torch.Tensor, normthreshold: float,
                 max_segments: Optional[int] = None, quantizer=None):
        """hidden ``[B,T,768]``, (seg, nseg, feats) as returned by ``HubertEncoderHIP.segment`` -> ``(input [B,T,out],
        averaged_target_hidden_states [B,T,768])`` — the tensors named so at segment_synthesis.py:115,138-139.
        ``quantizer``: the optional substitution inside the averaging loop (segment_synthesis.py:121-125): every segment
        mean is replaced by its nearest codebook entry (``get_indices`` -> ``get_output_from_indices``) before it is
        broadcast to its frames and fed to the MLP; a ``KMQuantizer`` or a ``ResidualKMQuantizer`` (the sum of both codebooks)."""
        B, T, D = hidden.shape
        if D != self.input_dim:
            raise ValueError("hidden dim %d != MLP input dim %d" % (D, self.input_dim))
        S = int(max_segments) if max_segments is not None else max(1, int(nseg.max().item()))
        S = min(max(S, 1), T)
        if quantizer is not None:
            # only the first S slots per utterance are ever read; slots beyond an utterance's own count are ignored by
            # sylber_condition, so they may hold anything (NaN rows of unused slots map to index 0 and stay unused)
            head = torch.nan_to_num(feats[:, :S].contiguous())
            q = quantizer.decode(quantizer.get_indices(head))
            feats = feats.clone()
            feats[:, :S] = q
        cond = torch.empty(B, T, self.output_dim, dtype=torch.float32, device=self.device)
        avg = torch.empty(B, T, D, dtype=torch.float32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_condition_workspace_floats(self.handle, B, S)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_condition(self.handle, _vp(hidden), _vp(seg), _vp(nseg), _vp(feats), B, T, S,
                                                 ctypes.c_float(float(np.float32(normthreshold))), _vp(avg), _vp(cond), _vp(ws),
                                                 _stream(self.device)), "sylber_condition")
        return cond, avg

    def packed(self, hidden: torch.Tensor, offsets: Sequence[int], frames: Sequence[int], seg: torch.Tensor, nseg: torch.Tensor,
               feats: torch.Tensor, normthreshold: float, max_segments: Optional[int] = None, quantizer=None) -> torch.Tensor:
        """``__call__`` for a packed batch (``sylber_condition_packed``): hidden ``[offsets[-1], 768]`` of ``forward_packed`` (clip b's frame t
        at row ``offsets[b] + t``), (seg, nseg, feats) of ``segment_packed`` (``[B, K, ...]``, relative to each clip's start) ->
        the conditioning input ``[sum frames, out]`` of each clip's own frames, back to back: row for row what ``__call__`` computes
        for the clip's frames in batch-invariant mode (the same silence mask and quantizer substitution)."""
        B, K, D = feats.shape
        fl = [int(f) for f in frames]
        ol = [int(o) for o in offsets]
        if D != self.input_dim:
            raise ValueError("feature dim %d != MLP input dim %d" % (D, self.input_dim))
        if len(fl) != B or len(ol) != B + 1:
            raise ValueError("need %d frame counts and %d offsets, got %d and %d" % (B, B + 1, len(fl), len(ol)))
        S = int(max_segments) if max_segments is not None else max(1, int(nseg.max().item()))
        S = min(max(S, 1), K)
        if quantizer is not None:
            head = torch.nan_to_num(feats[:, :S].contiguous())
            q = quantizer.decode(quantizer.get_indices(head))
            feats = feats.clone()
            feats[:, :S] = q
        cond = torch.empty(sum(fl), self.output_dim, dtype=torch.float32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_condition_packed_workspace_floats(self.handle, B, S)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_condition_packed(self.handle, _vp(hidden), (ctypes.c_int32 * (B + 1))(*ol), (ctypes.c_int32 * B)(*fl), B,
                                                        _vp(seg), _vp(nseg), _vp(feats.contiguous()), K, S,
                                                        ctypes.c_float(float(np.float32(normthreshold))), None, _vp(cond), _vp(ws),
                                                        _stream(self.device)), "sylber_condition_packed")
        return cond

    def from_features(self, features: torch.Tensor) -> torch.Tensor:
        """the ``features is not None`` branch of ``resynthesize`` (segment_synthesis.py:135-140): ``features [B,T,768]``
        (already averaged / decoded by the caller) -> ``input [B,T,out]`` = MLP(features) with the frames whose
        ``((features**2).sum(-1))**.5 < 1e-4`` zeroed (threshold and missing 1e-8 exactly as the reference)."""
        lead = tuple(features.shape[:-1])
        x = features.reshape(-1, features.shape[-1]).to(self.device, torch.float32).contiguous()
        if x.shape[1] != self.input_dim:
            raise ValueError("feature dim %d != MLP input dim %d" % (x.shape[1], self.input_dim))
        rows = x.shape[0]
        cond = torch.empty(rows, self.output_dim, dtype=torch.float32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_condition_workspace_floats(self.handle, rows, 1)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_condition_features(self.handle, _vp(x), rows, _vp(cond), _vp(ws), _stream(self.device)),
                       "sylber_condition_features")
        return cond.reshape(lead + (self.output_dim,))

    def from_units(self, codebooks: Sequence[torch.Tensor], units: torch.Tensor, spans: torch.Tensor, nunits: torch.Tensor, T: Optional[int],
                   frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``sylber_condition_units``: the conditioning input of syllable units -> ``[B, T, out]``, bitwise
        ``from_features(expand_feature(decode(units), durations))``.  ``T=None`` with ``frames``: a packed batch
        (``sylber_condition_units_packed``) -> ``[sum frames, out]``, each clip's own frames back to back, row for row the padded call's
        with ``T = max(frames)``.  ``codebooks``: one or two ``[K, 768]`` fp32 device tensors
        (decode sums them); ``units [B, S, len(codebooks)]``, ``spans [B, S, 2]`` (frames [start, end) of each unit), ``nunits [B]``,
        ``frames [B]`` (optional): int32 device tensors.  Bad ids, spans or counts raise ``SylberHipError``."""
        if not 1 <= len(codebooks) <= 2:
            raise ValueError("one or two codebooks")
        c1 = codebooks[0]
        c2 = codebooks[1] if len(codebooks) > 1 else None
        i32 = lambda t: torch.as_tensor(t).to(self.device, torch.int32).contiguous()   # noqa: E731
        units, spans, nunits = i32(units), i32(spans), i32(nunits)
        frames = i32(frames) if frames is not None else None
        if units.dim() != 3:
            raise ValueError("units must be [B, S, ncb]")
        B, S, ncb = units.shape
        if ncb != len(codebooks) or tuple(spans.shape) != (B, S, 2) or tuple(nunits.shape) != (B,):
            raise ValueError("units [B, S, %d], spans [B, S, 2] and nunits [B] expected, got %s, %s, %s"
                             % (len(codebooks), tuple(units.shape), tuple(spans.shape), tuple(nunits.shape)))
        for c in codebooks:
            if c.dim() != 2 or c.shape[1] != self.input_dim:
                raise ValueError("codebooks must be [K, %d]" % self.input_dim)
        if T is None:                      # packed: each clip's own frames, back to back
            if frames is None:
                raise ValueError("a packed call (T=None) needs frames")
            fl = [int(f) for f in frames.cpu().tolist()]
            if len(fl) != B:
                raise ValueError("need %d frame counts, got %d" % (B, len(fl)))
            cond = torch.empty(sum(fl), self.output_dim, dtype=torch.float32, device=self.device)
            ws = torch.empty(int(self.lib.sylber_condition_packed_workspace_floats(self.handle, B, S)), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.sylber_condition_units_packed(self.handle, _vp(c1), c1.shape[0], _vp(c2) if c2 is not None else None,
                                                                  c2.shape[0] if c2 is not None else 0, _vp(units), _vp(spans), _vp(nunits),
                                                                  (ctypes.c_int32 * B)(*fl), B, S, _vp(cond), _vp(ws), _stream(self.device)),
                           "sylber_condition_units_packed")
            return cond
        cond = torch.empty(B, int(T), self.output_dim, dtype=torch.float32, device=self.device)
        ws = torch.empty(int(self.lib.sylber_condition_units_workspace_floats(self.handle, B, S)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sylber_condition_units(self.handle, _vp(c1), c1.shape[0], _vp(c2) if c2 is not None else None,
                                                       c2.shape[0] if c2 is not None else 0, _vp(units), _vp(spans), _vp(nunits),
                                                       _vp(frames) if frames is not None else None, B, int(T), S, _vp(cond), _vp(ws),
                                                       _stream(self.device)), "sylber_condition_units")
        return cond
