"""Drop-in ``Segmenter`` for the MI355X: same constructor and ``__call__`` contract as the reference
(sylber/model/sylber.py:28-138), with the arithmetic on hand-written HIP kernels behind the C-ABI of
include/sylber_hip.h.  Host code stays Python on PyTorch-ROCm (device memory, streams)."""
from __future__ import annotations

import ctypes
import math
import os
import collections
import threading
import time
import weakref
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .ingest import ingest_file
from .weights import (NUM_LAYERS, expected_shapes, fold_pos_conv_weight, normalize_keys, synthetic_state_dict)

FRAME_RATE = 50  # sylber.py:132
SLOT_SAMPLES = 320  # waveform samples per frame of a packed batch's slot (the conv stack's total stride)
PACKED_PRECISIONS = ("bf16", "fp16")


def _ptr(t: torch.Tensor):
    return ctypes.cast(t.data_ptr(), _lib.c_float_p)


def _stream_ptr(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def load_wav_file(path: str) -> torch.Tensor:
    """PCM ``.wav`` -> float32 [C, N] in [-1, 1) on the HOST (what torchaudio.load returns at sylber.py:83), 16 kHz
    files only.  Kept for tests and tools; ``Segmenter.__call__(wav_file=...)`` ingests on the device instead
    (sylber_amd/ingest.py: decode + resample + normalise in HIP)."""
    from .ingest import read_pcm
    pcm = read_pcm(path)
    if pcm.sample_rate != 16000:
        raise NotImplementedError("load_wav_file is the host-side 16 kHz reader (got %d Hz); use sylber_amd.ingest" % pcm.sample_rate)
    raw, width = pcm.data, pcm.sample_width
    if width == 2:
        x = raw.view("<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = raw.view("<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (raw.astype(np.float32) - 128.0) / 128.0
    else:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    return torch.from_numpy(x.reshape(-1, pcm.channels).T.copy())


class PinnedOutputPool:
    """Persistent page-locked host blocks for the results of ``Segmenter.__call__`` (reference: the D2H of
    sylber.py:122-138, where ``.cpu().numpy()`` lands in pageable memory).

    Page-locking is the expensive part of a pinned allocation (tens to hundreds of ms for the 49 MB of hidden states of
    a 32 x 10 s batch), so blocks are allocated once and LEASED: a call's numpy results are views of one block, and the
    block returns to the pool when the last of those views is garbage collected (a finalizer on the owning ndarray --
    every numpy view of it keeps that owner alive through ``.base``).  Nothing is ever overwritten while a caller can
    still see it.  At most ``max_leased`` blocks are out at a time: beyond that (a corpus loop that keeps every result)
    ``lease`` returns None and the caller falls back to pageable per-utterance copies, so retained results never pin
    more than ``max_leased`` batches of host memory."""

    GRANULE = 1 << 20

    def __init__(self, max_leased: int = 4, alloc=None):
        self.max_leased = int(max_leased)
        self._free: List[torch.Tensor] = []
        self._leased = 0
        self._lock = threading.Lock()
        # blocks handed back by finalizers.  A finalizer can run at ANY allocation point -- including inside lease() on the
        # same thread while it holds the (non-reentrant) lock, when a collection frees owner arrays caught in a reference
        # cycle -- so the release path takes no lock: deque.append is atomic, and lease() drains the deque under the lock
        self._returned = collections.deque()
        self._alloc = alloc or _pinned            # (tests inject pageable memory)
        self.allocations = 0                      # page-locking events so far (tests / bench: must stop growing)

    def _release(self, blk: torch.Tensor) -> None:
        self._returned.append(blk)

    def _drain(self) -> None:                     # (lock held)
        while True:
            try:
                blk = self._returned.popleft()
            except IndexError:
                return
            self._leased -= 1
            self._free.append(blk)

    @property
    def leased(self) -> int:
        with self._lock:
            self._drain()
            return self._leased

    def trim(self) -> None:
        """drop free blocks beyond what ``max_leased`` can ever hand out again (after a temporarily raised budget: Segmenter.stream)"""
        with self._lock:
            self._drain()
            while self._free and len(self._free) + self._leased > self.max_leased:
                self._free.pop(0)

    def lease(self, nbytes: int):
        """-> (owner ndarray uint8 [cap], block tensor) or None when ``max_leased`` blocks are already out"""
        with self._lock:
            self._drain()
            if self._leased >= self.max_leased:
                return None
            pick = None
            for i, b in enumerate(self._free):
                if b.numel() >= nbytes and (pick is None or b.numel() < self._free[pick].numel()):
                    pick = i
            blk = self._free.pop(pick) if pick is not None else None
            if blk is None and len(self._free) + self._leased >= self.max_leased and self._free:
                self._free.pop(0)                 # too small for this batch shape: let it go instead of hoarding
            self._leased += 1
        if blk is None:
            cap = (int(nbytes) + self.GRANULE - 1) // self.GRANULE * self.GRANULE
            try:
                blk = self._alloc(cap)
            except BaseException:
                with self._lock:
                    self._leased -= 1
                raise
            self.allocations += 1
        owner = blk.numpy()
        weakref.finalize(owner, self._release, blk)
        return owner, blk


def _pinned(nbytes: int) -> torch.Tensor:
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _pad_rows(stage_np: np.ndarray, rows, lengths, lo: int, hi: int) -> None:
    """rows [lo, hi) of a batch into the host staging view, zero padded to its width (numpy's copy releases the GIL)"""
    for i in range(lo, hi):
        src = rows[i].detach()
        stage_np[i, : lengths[i]] = (src if src.dtype == torch.float32 else src.to(torch.float32)).numpy()
        stage_np[i, lengths[i]:] = 0.0


def packed_layout(lengths: Sequence[int]):
    """The slots of a packed batch (``sylber_packed_layout``; host only, no GPU): per-clip sample counts -> ``(offsets, frames)``, int32
    arrays of B + 1 slot offsets in frames (``offsets[-1]`` = the batch's total frames) and of each clip's own frame count.  Clip b's
    waveform goes to sample ``SLOT_SAMPLES * offsets[b]`` of the packed buffer, its hidden states come back as rows
    ``[offsets[b], offsets[b] + frames[b])``.  ValueError for an empty batch, a clip below 400 samples or a batch too long for 32-bit offsets."""
    lib = _lib.load()
    n = [int(x) for x in lengths]
    B = len(n)
    if B < 1:
        raise ValueError("a packed batch needs at least one clip")
    if any(x < 400 or x > 2 ** 31 - 1 for x in n):
        raise ValueError("every clip of a packed batch needs 400 .. 2^31 - 1 samples, got %s" % n)
    off, fr = (ctypes.c_int32 * (B + 1))(), (ctypes.c_int32 * B)()
    if lib.sylber_packed_layout((ctypes.c_int32 * B)(*n), B, off, fr) != 0:
        raise ValueError(lib.sylber_last_error().decode())
    return np.frombuffer(off, dtype=np.int32).copy(), np.frombuffer(fr, dtype=np.int32).copy()


def _stage_packed(stage_np: np.ndarray, rows, lengths, offsets, lo: int, hi: int) -> None:
    """clips [lo, hi) of a batch into the flat host staging view of a packed batch: clip i at sample ``SLOT_SAMPLES * offsets[i]``, zeros
    to the end of its slot (numpy's copy releases the GIL)"""
    for i in range(lo, hi):
        a, e = SLOT_SAMPLES * int(offsets[i]), SLOT_SAMPLES * int(offsets[i + 1])
        src = rows[i].detach()
        stage_np[a:a + lengths[i]] = (src if src.dtype == torch.float32 else src.to(torch.float32)).numpy()
        stage_np[a + lengths[i]:e] = 0.0


class _BlockLayout:
    """Byte layout of the host block one batch's results land in: [hidden states | tables | pooled features | counts], every part
    256-byte aligned, ``kcap`` segment slots per utterance.  The views work on the torch uint8 block (the D2H copies' targets) and
    on its numpy owner (what the caller gets)."""

    _TORCH = {np.float32: (torch.float32, 4), np.int32: (torch.int32, 4), np.int64: (torch.int64, 8)}

    def __init__(self, B: int, T: int, D: int, kcap: int, with_hidden: bool, with_feats: bool, frames: Optional[Sequence[int]] = None):
        def al(n):
            return (n + 255) & ~255
        self.B, self.T, self.D, self.kcap = B, T, D, kcap
        self.with_hidden, self.with_feats = with_hidden, with_feats
        # frames (packed batches): the hidden part holds only each clip's own frames, back to back ([sum(frames), D])
        self.frames = None if frames is None else [int(f) for f in frames]
        self.starts = None if frames is None else np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        hrows = B * T if frames is None else int(self.starts[-1])
        self.o_seg = al(hrows * D * 4) if with_hidden else 0
        self.o_feat = self.o_seg + al(B * kcap * 2 * 8)
        self.o_cnt = self.o_feat + (al(B * kcap * D * 4) if with_feats else 0)
        self.nbytes = self.o_cnt + al(B * 4)

    @classmethod
    def _view(cls, buf, off: int, dtype, shape):
        tdt, size = cls._TORCH[dtype]
        n = math.prod(shape) * size
        if torch.is_tensor(buf):
            return buf[off:off + n].view(tdt).view(shape)
        return buf[off:off + n].view(dtype).reshape(shape)

    def hidden(self, buf):
        if not self.with_hidden:
            return None
        if self.frames is not None:
            return self._view(buf, 0, np.float32, (int(self.starts[-1]), self.D))
        return self._view(buf, 0, np.float32, (self.B, self.T, self.D))

    def clip_hidden(self, buf):
        """packed layout: one [frames[b], D] view per clip"""
        h = self.hidden(buf)
        return None if h is None else [h[self.starts[b]:self.starts[b + 1]] for b in range(self.B)]

    def counts(self, buf):
        return self._view(buf, self.o_cnt, np.int32, (self.B,))

    def tables(self, buf, k: Optional[int] = None):
        """(segments [B, k, 2] int64, pooled features [B, k, D] float32 or None), packed at the start of their parts (k <= kcap)"""
        k = self.kcap if k is None else k
        return (self._view(buf, self.o_seg, np.int64, (self.B, k, 2)),
                self._view(buf, self.o_feat, np.float32, (self.B, k, self.D)) if self.with_feats else None)


def _fetch_tables(seg: torch.Tensor, feats: Optional[torch.Tensor], k: int, alloc=_pinned):
    """The tables of a batch with more segments than its block has slots: the first ``k`` slots of the device tables (and pooled
    features) into a private block of their own, on the current stream.  -> their numpy views, valid once that stream is synchronised."""
    B, T = seg.shape[:2]
    lay = _BlockLayout(B, T, feats.shape[2] if feats is not None else 0, k, False, feats is not None)
    blk = alloc(lay.nbytes)
    seg_d, feat_d = lay.tables(blk)
    seg_d.copy_(seg[:, :k], non_blocking=True)
    if feat_d is not None:
        feat_d.copy_(feats[:, :k], non_blocking=True)
    return lay.tables(blk.numpy())


def _segment_list(seg_h: np.ndarray, nseg_h: np.ndarray) -> List[np.ndarray]:
    """host tables [B, k, 2] + counts [B] -> one int64 [n, 2] array per utterance (``np.array([])`` for none, sylber.py:134)"""
    return [seg_h[i, :int(n)].copy() if n > 0 else np.array([]) for i, n in enumerate(nseg_h)]


def _result_dicts(nseg_h, seg_h, feats_h=None, hidden_h=None, frames=None, in_second=True, handed=False) -> List[dict]:
    """The reference's per-utterance dicts (sylber.py:128-138) from host results: counts [B], tables [B, k, 2], optional pooled
    features [B, k, D] and hidden states [B, T, D] (cut to ``frames[i]`` frames when given).  ``handed``: the arrays belong to the
    caller (a leased or fresh block), so features and hidden states are returned as views of them; otherwise they are copied out."""
    outputs = []
    for i, segments in enumerate(_segment_list(seg_h, nseg_h)):
        n = len(segments)
        o = {"segments": segments * 1.0 / FRAME_RATE if in_second else segments}
        if feats_h is not None:
            o["segment_features"] = (feats_h[i, :n] if handed else feats_h[i, :n].copy()) if n > 0 else np.array([])
        if hidden_h is not None:
            hb = hidden_h[i] if frames is None else hidden_h[i, :frames[i]]
            o["hidden_states"] = hb if handed else hb.copy()
        outputs.append(o)
    return outputs


def _tables_to_host(seg: torch.Tensor, nseg: torch.Tensor):
    """-> (counts [B] int32, the first max(max(counts), 1) slots of the tables [B, k, 2] int64) on the host"""
    nseg_h = nseg.cpu().numpy()
    return nseg_h, seg[:, :max(int(nseg_h.max()), 1)].cpu().numpy()


class HubertEncoderHIP:
    """The (1) boundary of include/sylber_hip.h: weights -> handle, waveform batch -> hidden states."""

    supports_out = True          # forward / segment take caller-owned output tensors (out=): ShardedSegmenter.run_stream's buffer ring

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_layers: int = NUM_LAYERS, device: str = "cuda",
                 precision: str = "bf16"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SylberHipError("no MI355X visible to PyTorch-ROCm; the HIP path has no CPU fallback")
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.num_layers = num_layers
        self.precision = precision
        self._opts = {}
        sd = normalize_keys(state_dict)
        shapes = expected_shapes(num_layers)
        keep = {}

        def get(name):
            if name not in sd:
                raise KeyError("checkpoint is missing %s" % name)
            t = sd[name].detach().to("cpu", torch.float32).contiguous()
            if name in shapes and tuple(t.shape) != shapes[name]:
                raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), shapes[name]))
            keep[name] = t
            return _ptr(t)

        w = _lib.SylberWeights()
        w.num_layers = num_layers
        for i in range(7):
            w.conv_w[i] = get(f"feature_extractor.conv_layers.{i}.conv.weight")
        w.gn_w = get("feature_extractor.conv_layers.0.layer_norm.weight")
        w.gn_b = get("feature_extractor.conv_layers.0.layer_norm.bias")
        w.fp_ln_w = get("feature_projection.layer_norm.weight")
        w.fp_ln_b = get("feature_projection.layer_norm.bias")
        w.fp_w = get("feature_projection.projection.weight")
        w.fp_b = get("feature_projection.projection.bias")
        pos = fold_pos_conv_weight(sd)
        keep["pos"] = pos
        w.pos_w = _ptr(pos)
        w.pos_b = get("encoder.pos_conv_embed.conv.bias")
        w.enc_ln_w = get("encoder.layer_norm.weight")
        w.enc_ln_b = get("encoder.layer_norm.bias")
        for l in range(num_layers):
            p = f"encoder.layers.{l}."
            L = w.layers[l]
            L.q_w, L.q_b = get(p + "attention.q_proj.weight"), get(p + "attention.q_proj.bias")
            L.k_w, L.k_b = get(p + "attention.k_proj.weight"), get(p + "attention.k_proj.bias")
            L.v_w, L.v_b = get(p + "attention.v_proj.weight"), get(p + "attention.v_proj.bias")
            L.o_w, L.o_b = get(p + "attention.out_proj.weight"), get(p + "attention.out_proj.bias")
            L.ln1_w, L.ln1_b = get(p + "layer_norm.weight"), get(p + "layer_norm.bias")
            L.ff1_w, L.ff1_b = (get(p + "feed_forward.intermediate_dense.weight"),
                                get(p + "feed_forward.intermediate_dense.bias"))
            L.ff2_w, L.ff2_b = get(p + "feed_forward.output_dense.weight"), get(p + "feed_forward.output_dense.bias")
            L.ln2_w, L.ln2_b = get(p + "final_layer_norm.weight"), get(p + "final_layer_norm.bias")
        h = ctypes.c_void_p()
        prec = {"bf16": 0, "fp32": 1, "fp8": 2, "fp16": 3, "mixed16": 4, "split16": 5}[precision]
        _lib.check(self.lib.sylber_create(ctypes.byref(w), self.device.index or 0, prec, ctypes.byref(h)),
                   "sylber_create")                 # (the library restores the caller's current device itself)
        self.handle = h
        del keep

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.sylber_destroy(h)
            self.handle = None

    def num_frames(self, n_samples: int) -> int:
        return int(self.lib.sylber_num_frames(int(n_samples)))

    def padded_frames(self, n_samples: int) -> int:
        """frame pitch per utterance of the library's activation buffers (>= num_frames, multiple of 32)"""
        return int(self.lib.sylber_padded_frames(int(n_samples)))

    def set_option(self, key: int, value: int) -> None:
        """per-handle tuning / test override (include/sylber_hip.h SYLBER_OPT_*; value < 0 = automatic)"""
        _lib.check(self.lib.sylber_set_option(self.handle, int(key), int(value)), "sylber_set_option")
        self._opts[int(key)] = int(value)

    def forward(self, wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, stop_stage: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wav: [B, Lmax] float32 on this device, zero padded.  Returns [B, T, 768] float32 (device).

        ``stop_stage`` (include/sylber_hip.h sylber_set_stop_stage): 1 returns the conv features [B, T, 512], 2 / 3 + l the stream after
        the encoder LayerNorm / layer l.  Negative values are the taps of the front half: ``_lib.TAP_CONV0`` conv layer 0 alone,
        [B, 64 * padded_frames(Lmax), 512] (every row of its buffer); ``_lib.TAP_PROJ`` the projected residual stream and
        ``_lib.TAP_POSCONV`` the encoder LayerNorm's input, both [B, T, 768]; ``_lib.TAP_CONV(i)`` conv layer i = 1..6 alone,
        [B, padded_frames(Lmax) << (6 - i), 512] (every row of its buffer).  ``_lib.TAP_LAYER(l, k)`` is tap k (``_lib.LTAP_*``)
        inside encoder layer l: [B, T, _lib.LTAP_WIDTH[k]] (2304 = q | k | v, 3072 for FFN1, else 768).  In the fp8 precision the MXFP8
        buffers (QKV, CTX, LN1, FFN1) come back as [B, T, 2 W]: W values dequantised exactly, then W floats holding each element's block
        exponent s - 127 (``_lib.ltap_width``); the fp32 sums keep W, and so does QKV with ``_lib.OPT_FP8_ATTENTION`` at -1."""
        assert wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()
        B, Lmax = wav.shape
        T = self.num_frames(Lmax)
        if stop_stage == _lib.TAP_CONV0:
            shape = (B, 64 * self.padded_frames(Lmax), 512)
        elif _lib.TAP_CONV(7) <= stop_stage <= _lib.TAP_CONV(0):
            # (i = 0 and i = 7 are refused by the library below)
            shape = (B, self.padded_frames(Lmax) << max(6 + 1024 + stop_stage, 0), 512)
        elif stop_stage <= -8:
            # (an unknown k is refused by the library below)
            shape = (B, T, _lib.ltap_width(-stop_stage % 8, self.precision, self._opts.get(_lib.OPT_FP8_ATTENTION, 0) >= 0))
        else:
            shape = (B, T, 512 if stop_stage == 1 else 768)
        if out is None:
            out = torch.empty(*shape, dtype=torch.float32, device=wav.device)
        assert out.numel() >= shape[0] * shape[1] * shape[2]
        larr = None
        if lengths is not None:
            larr = (ctypes.c_int32 * B)(*[int(x) for x in lengths])
        _lib.check(self.lib.sylber_set_stop_stage(self.handle, int(stop_stage)), "sylber_set_stop_stage")
        cur = torch.cuda.current_stream(wav.device)
        use = cur
        if getattr(self, "_graph_stream", None) is not None and cur.cuda_stream == 0:
            # a hipGraph cannot be captured on the default stream: run on the handle's own stream, ordered both ways
            use = self._graph_stream
            use.wait_stream(cur)
        with torch.cuda.device(wav.device):
            st = self.lib.sylber_forward(self.handle, ctypes.c_void_p(wav.data_ptr()), larr, B, Lmax,
                                         ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(use.cuda_stream))
        if use is not cur:
            cur.wait_stream(use)
        self.lib.sylber_set_stop_stage(self.handle, 0)
        _lib.check(st, "sylber_forward")
        return out

    def conv0_scale_shift(self, B: int) -> np.ndarray:
        """test aid: conv0's GroupNorm table of the last forward (of B utterances), [B, 512, 2] float32 = (scale, shift) per channel"""
        out = np.empty((int(B), 512, 2), dtype=np.float32)
        _lib.check(self.lib.sylber_debug_conv0_scale_shift(self.handle, int(B), out.ctypes.data_as(ctypes.c_void_p)),
                   "sylber_debug_conv0_scale_shift")
        return out

    def set_batches_in_flight(self, n: int) -> None:
        """tell the handle whether it owns the chip (n = 1, the default: a synchronous caller) or shares it with other in-flight batches on other
        handles / streams (n >= 2: bench.py's pipeline, ShardedSegmenter's engines).  Only the GEMM tile choice depends on it
        (SYLBER_OPT_GEMM_MODEL, include/sylber_hip.h); results are bit-identical."""
        self.set_option(12, 5 if int(n) >= 2 else 0)

    def set_graph_mode(self, enable: bool = True) -> None:
        """Replay the forward's ~110 kernel launches from a captured hipGraph (per (B, Lmax, input, output buffers);
        captured on the second call with the same key).  For launch-bound small batches; pass ``out=`` and reuse the
        input buffer so that the key repeats."""
        _lib.check(self.lib.sylber_set_graph_mode(self.handle, 1 if enable else 0), "sylber_set_graph_mode")
        self._graph_stream = torch.cuda.Stream(device=self.device) if enable else None

    def _check_packed(self, what: str) -> None:
        """ValueError, before any launch, for what the packed path does not cover"""
        if self.precision not in PACKED_PRECISIONS:
            raise ValueError("%s: packed batches run in precision %s only (this encoder: %r)" % (what, " / ".join(map(repr, PACKED_PRECISIONS)),
                                                                                                   self.precision))
        if getattr(self, "_graph_stream", None) is not None:
            raise ValueError("%s: packed batches do not run in graph mode (set_graph_mode(False))" % what)
        if self._opts.get(_lib.OPT_SEGMENT, 0) < 0:
            raise ValueError("%s: packed boundary detection needs the wide segmenter (SYLBER_OPT_SEGMENT = 0, not -1)" % what)
        # exactly the settings sylber_forward_packed refuses: sylber_set_option stores a non-zero queries-per-wave state only for the
        # values 32 and 64 (any other value selects the automatic kernel), and a non-zero conv0 switch for every value > 0
        if (self._opts.get(_lib.OPT_ATTN_QUERIES_PER_WAVE, 0) in (32, 64) or self._opts.get(_lib.OPT_CONV0_VALU, 0) > 0):
            raise ValueError("%s: packed batches need SYLBER_OPT_ATTN_QUERIES_PER_WAVE and SYLBER_OPT_CONV0_VALU at their defaults" % what)

    def forward_packed_raw(self, wav: torch.Tensor, lengths: Sequence[int], out: Optional[torch.Tensor] = None, layout=None) -> torch.Tensor:
        """A staged packed batch (``packed_layout``): wav [SLOT_SAMPLES * offsets[-1]] float32 on this device, clip b at sample
        ``SLOT_SAMPLES * offsets[b]``, zeros to the end of its slot; lengths = the clips' sample counts.  Returns the hidden states
        [offsets[-1], 768] float32 (device): clip b's are rows [offsets[b], offsets[b] + frames[b]), bit-identical to a forward of it alone.
        ``layout``: ``packed_layout(lengths)`` when the caller has it already."""
        self._check_packed("forward_packed")
        n = [int(x) for x in lengths]
        offsets, _ = packed_layout(n) if layout is None else layout
        P = int(offsets[-1])
        assert wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous() and wav.numel() == SLOT_SAMPLES * P
        if out is None:
            out = torch.empty(P, 768, dtype=torch.float32, device=wav.device)
        assert out.is_contiguous() and out.numel() >= P * 768
        with torch.cuda.device(wav.device):
            st = self.lib.sylber_forward_packed(self.handle, ctypes.c_void_p(wav.data_ptr()), (ctypes.c_int32 * len(n))(*n), len(n),
                                                ctypes.c_void_p(out.data_ptr()), _stream_ptr(wav.device))
        _lib.check(st, "sylber_forward_packed")
        return out

    def forward_packed(self, wavs: Sequence[torch.Tensor]):
        """Clips of different lengths (1-D tensors, host or device) as ONE packed batch, no padding to the longest: each gets a slot of its
        own frames rounded up to 64 (``packed_layout``).  Returns ``(hidden [offsets[-1], 768] device, offsets [B + 1], frames [B])``;
        clip b's hidden states are ``hidden[offsets[b]:offsets[b] + frames[b]]``, bit-identical to a forward of that clip alone."""
        self._check_packed("forward_packed")
        rows = [torch.as_tensor(w).reshape(-1) for w in wavs]
        lengths = [int(r.numel()) for r in rows]
        offsets, frames = packed_layout(lengths)
        wav = torch.zeros(SLOT_SAMPLES * int(offsets[-1]), dtype=torch.float32, device=self.device)
        for i, r in enumerate(rows):
            a = SLOT_SAMPLES * int(offsets[i])
            wav[a:a + lengths[i]] = r.to(self.device, torch.float32)
        return self.forward_packed_raw(wav, lengths), offsets, frames

    def segment_packed(self, hidden: torch.Tensor, lengths: Sequence[int], norm_threshold: float, merge_threshold: float,
                       with_features: bool = True, out=None, layout=None):
        """Boundary detection of a packed batch (``sylber_segment_packed``): hidden [offsets[-1], 768] of ``forward_packed``, lengths = the
        clips' sample counts.  Clip b is segmented and pooled as its own frames alone.  Returns (segments [B, kcap, 2] int64 relative to
        the clip's start, nseg [B] int32, feats [B, kcap, 768] or None), kcap = max(frames).  Same stream rules as ``segment``."""
        self._check_packed("segment_packed")
        n = [int(x) for x in lengths]
        offsets, frames = packed_layout(n) if layout is None else layout
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous() and hidden.numel() >= int(offsets[-1]) * 768
        B, K, D = len(n), int(frames.max()), 768
        if out is not None:
            seg, nseg, feats = out
        else:
            seg = torch.empty(B, K, 2, dtype=torch.int64, device=hidden.device)
            nseg = torch.empty(B, dtype=torch.int32, device=hidden.device)
            feats = torch.empty(B, K, D, dtype=torch.float32, device=hidden.device) if with_features else None
        with torch.cuda.device(hidden.device):
            st = self.lib.sylber_segment_packed(self.handle, ctypes.c_void_p(hidden.data_ptr()), (ctypes.c_int32 * B)(*n), B,
                                                ctypes.c_float(float(np.float32(norm_threshold))),
                                                ctypes.c_float(float(np.float32(merge_threshold))),
                                                ctypes.c_void_p(seg.data_ptr()), ctypes.c_void_p(nseg.data_ptr()),
                                                ctypes.c_void_p(feats.data_ptr()) if feats is not None else None, _stream_ptr(hidden.device))
        _lib.check(st, "sylber_segment_packed")
        return seg, nseg, feats

    def gather_packed(self, hidden: torch.Tensor, lengths: Sequence[int], out: Optional[torch.Tensor] = None, layout=None) -> torch.Tensor:
        """each clip's own rows of a packed forward's hidden states, back to back (``sylber_packed_gather``): [sum(frames), 768] on the
        device, on the current stream -- one device-to-host copy then fetches exactly the clips' frames"""
        n = [int(x) for x in lengths]
        _, frames = packed_layout(n) if layout is None else layout
        rows = int(frames.sum())
        if out is None:
            out = torch.empty(rows, 768, dtype=torch.float32, device=hidden.device)
        assert hidden.is_cuda and hidden.is_contiguous() and out.is_contiguous() and out.numel() >= rows * 768
        with torch.cuda.device(hidden.device):
            st = self.lib.sylber_packed_gather(ctypes.c_void_p(hidden.data_ptr()), (ctypes.c_int32 * len(n))(*n), len(n),
                                               ctypes.c_void_p(out.data_ptr()), _stream_ptr(hidden.device))
        _lib.check(st, "sylber_packed_gather")
        return out[:rows]

    def set_per_utterance(self, enable: bool = True) -> None:
        """batch-invariant encoder (include/sylber_hip.h SYLBER_OPT_PER_UTTERANCE): conv0's GroupNorm statistics of every row over its
        own length, so ``forward(...)[b, :T_b]`` is bit-identical to a forward of that clip alone"""
        self.set_option(_lib.OPT_PER_UTTERANCE, 1 if enable else 0)

    def frame_counts(self, lengths: Sequence[int]) -> List[int]:
        """frames of each row's own length (``num_frames`` per row)"""
        return [self.num_frames(int(n)) for n in lengths]

    def segment(self, hidden: torch.Tensor, norm_threshold: float, merge_threshold: float, with_features: bool = True,
                out=None, frames: Optional[Sequence[int]] = None):
        """hidden: [B, T, 768] float32 device.  Returns (segments [B,T,2] int64, nseg [B] int32, feats [B,T,768]).
        Runs on the CURRENT torch stream; it touches no encoder workspace, so a caller may run it on a side
        stream concurrently with the next batch's forward; it uses the handle's own scratch slab (frame norms, slot table), so the
        segment calls of one handle must be ordered on one stream.
        ``frames``: each row's own frame count (``sylber_segment_frames``): row b is segmented and pooled as ``hidden[b, :frames[b]]``
        alone would be, frames past it are never read.  Counts outside ``[1, T]`` raise ValueError."""
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous()
        B, T, D = hidden.shape
        farr = None
        if frames is not None:
            fl = [int(f) for f in frames]
            if len(fl) != B:
                raise ValueError("frames must have one count per row (%d), got %d" % (B, len(fl)))
            if any(f < 1 or f > T for f in fl):
                raise ValueError("frame counts must be in [1, %d], got %s" % (T, fl))
            farr = (ctypes.c_int32 * B)(*fl)
        if out is not None:
            seg, nseg, feats = out
        else:
            seg = torch.empty(B, T, 2, dtype=torch.int64, device=hidden.device)
            nseg = torch.empty(B, dtype=torch.int32, device=hidden.device)
            feats = torch.empty(B, T, D, dtype=torch.float32, device=hidden.device) if with_features else None
        args = (B, T, D, ctypes.c_float(float(np.float32(norm_threshold))), ctypes.c_float(float(np.float32(merge_threshold))),
                ctypes.c_void_p(seg.data_ptr()), ctypes.c_void_p(nseg.data_ptr()),
                ctypes.c_void_p(feats.data_ptr()) if feats is not None else None, _stream_ptr(hidden.device))
        with torch.cuda.device(hidden.device):
            if farr is None:
                st = self.lib.sylber_segment(self.handle, ctypes.c_void_p(hidden.data_ptr()), *args)
            else:
                st = self.lib.sylber_segment_frames(self.handle, ctypes.c_void_p(hidden.data_ptr()), farr, *args)
        _lib.check(st, "sylber_segment" if farr is None else "sylber_segment_frames")
        return seg, nseg, feats

    def segment_batch(self, input_values, attention_mask, norm_threshold: float, merge_threshold: float, per_row: bool):
        """A padded waveform batch ``[B, N]`` (or one ``[N]`` clip) and its optional 0/1 ``attention_mask`` -> forward, each row's own
        frame count, segmentation (``per_row``: over each row's own frames, batch-invariant mode), and the counts plus the first
        ``max(max(nseg), 1)`` table slots on the host.  Returns ``(hidden, frames, seg, nseg, feats, nseg_h, seg_h)``."""
        x = torch.as_tensor(input_values).to(self.device, torch.float32)
        if x.dim() == 1:
            x = x[None]
        x = x.contiguous()
        lengths = None if attention_mask is None else [int(v) for v in torch.as_tensor(attention_mask).sum(-1).tolist()]
        hidden = self.forward(x, lengths)
        frames = self.frame_counts(lengths if lengths is not None else [x.shape[1]] * x.shape[0])
        seg, nseg, feats = self.segment(hidden, norm_threshold, merge_threshold, frames=frames if per_row else None)
        return (hidden, frames, seg, nseg, feats) + _tables_to_host(seg, nseg)

    def set_profiling(self, on: bool) -> None:
        self.lib.sylber_set_profiling(self.handle, 1 if on else 0)

    def get_profile(self) -> Dict[str, float]:
        cap = 64
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        n = self.lib.sylber_get_profile(self.handle, names, ms, cap)
        return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}

    def workspace_bytes(self) -> int:
        return int(self.lib.sylber_workspace_bytes(self.handle))

    def fp16_audit(self, start: bool = False):
        """fp16 headroom audit (include/sylber_hip.h SYLBER_OPT_FP16_AUDIT; precision "fp16" / "mixed16" only -- the other modes have nothing to
        saturate).  ``fp16_audit(start=True)`` (re)starts it: from then on every forward scans each 16-bit activation buffer behind its
        producer.  ``fp16_audit()`` returns ``{stage: {"saturated": values clamped at +-65504, "max_abs": largest magnitude}}`` since the
        start (synchronises the device), or ``{}`` when it never ran.  A non-zero ``saturated`` anywhere means the checkpoint does not fit
        IEEE half there: use "bf16" or "split16"."""
        if start:
            self.set_option(10, 1)
            return None
        cap = 32
        names = (ctypes.c_char_p * cap)()
        sat = (ctypes.c_uint32 * cap)()
        mx = (ctypes.c_float * cap)()
        n = self.lib.sylber_get_fp16_audit(self.handle, names, sat, mx, cap)
        if n < 0:
            _lib.check(1, "sylber_get_fp16_audit")
        return {names[i].decode(): {"saturated": int(sat[i]), "max_abs": float(mx[i])} for i in range(n)}


class Segmenter:
    """Same signature as the reference's ``Segmenter`` (sylber/model/sylber.py:30-39, 63)."""

    def __init__(self, model_ckpt="sylber", speech_upstream="facebook/hubert-base-ls960", ema_decay=0.999,
                 encoding_layer=9, merge_threshold=0.8, norm_threshold=2.6, device="cuda", **kwargs):
        self.encoding_layer = encoding_layer
        self.enc_dim = 768
        # packed batches (off by default): a ragged batch runs without padding to its longest clip -- each clip in a slot of its own
        # frames rounded up to 64 (packed_layout) -- with batch_invariant=True's results, bit for bit (bf16 and fp16 only)
        self.packed = bool(kwargs.get("packed", False))
        if self.packed and kwargs.get("precision", "bf16") not in PACKED_PRECISIONS:
            raise ValueError("packed=True supports precision %s only (got %r)" % (" / ".join(map(repr, PACKED_PRECISIONS)), kwargs.get("precision")))
        state_dict = self._load_state_dict(model_ckpt, encoding_layer)
        if "cuda" not in str(device):
            raise _lib.SylberHipError("sylber_amd.Segmenter runs on the MI355X only (device=%r)" % (device,))
        self.speech_model = HubertEncoderHIP(state_dict, num_layers=encoding_layer, device=device,
                                             precision=kwargs.get("precision", "bf16"))
        self.device = str(self.speech_model.device)
        # __call__ is synchronous: ONE batch in flight on this handle, where the residual GEMMs' K loops prefetching all three
        # fragment columns of the residual rows is the faster setting (-1.0 % of the forward; with two batches in flight on
        # two handles, as bench.py's pipeline runs, one column is: profiles/r04_resln_prefetch.md).  Bit-identical either way.
        self._resln_prefetch = int(kwargs.get("resln_prefetch", 3))
        self.speech_model.set_option(6, self._resln_prefetch)
        # batch-invariant mode (off by default): every clip of a batch gets exactly the results it gets alone -- GroupNorm statistics
        # over its own length (SYLBER_OPT_PER_UTTERANCE), segmentation over its own frames (sylber_segment_frames), hidden states cut to them
        self.batch_invariant = bool(kwargs.get("batch_invariant", False)) or self.packed
        if self.batch_invariant:
            self.speech_model.set_per_utterance(True)
        self.norm_threshold = norm_threshold
        self.merge_threshold = merge_threshold
        # where __call__'s numpy results live: "pinned" (default) = views of leased page-locked blocks, at most
        # `max_pinned_batches` batches outstanding, pageable copies beyond that; "pageable" = always ordinary arrays
        # (what the reference returns).  See PinnedOutputPool.
        self.output_memory = kwargs.get("output_memory", "pinned")
        if self.output_memory not in ("pinned", "pageable"):
            raise ValueError("output_memory must be 'pinned' or 'pageable'")
        self.out_pool = PinnedOutputPool(max_leased=int(kwargs.get("max_pinned_batches", 4)))
        # host padding of tensor inputs (encode_batch).  tools/pad_probe.py on the 256-cpu boxes: the 20 MB copy of a 32 x 10 s batch into the
        # page-locked staging buffer takes 0.49 ms on one thread, 0.36-0.44 on two, MORE on four / eight / sixteen (0.58 / 0.93 / 1.25: waking
        # pool threads costs more than the copy they take over; numpy slice assignment and ctypes.memmove alike)
        self._fill_threads = max(1, int(kwargs.get("host_pad_threads", 2)))
        self._fill_groups = max(1, int(kwargs.get("host_pad_groups", 8)))       # row groups the padding + H2D of a batch is cut into (H2D of group g under the padding of g + 1)
        self._kcap_seen = 128                                                    # segment slots per utterance the next block is sized for
        self._kcap_recent = collections.deque(maxlen=16)                         # per-batch maxima of the last 16 batches (sizing decays with them)
        # which keys of the reference's dict (sylber.py:134-138) a call returns.  Default = all three, the reference's contract.  A caller
        # that consumes only the tables / pooled features (tokenisation, the resynthesis front half) can drop "hidden_states": that skips
        # the 49 MB device-to-host copy of a 32 x 10 s batch (0.87 ms of a 7.9 ms call) and its page-locked block (round 6)
        outs = tuple(kwargs.get("outputs", ("segments", "segment_features", "hidden_states")))
        bad = [o for o in outs if o not in ("segments", "segment_features", "hidden_states")]
        if bad or "segments" not in outs:
            raise ValueError("outputs must contain 'segments' and may add 'segment_features', 'hidden_states' (got %r)" % (outs,))
        self.outputs = outs
        self._want_hidden = "hidden_states" in outs
        self._want_feats = "segment_features" in outs

    @staticmethod
    def _load_state_dict(model_ckpt, encoding_layer):
        if model_ckpt is None:
            # the reference keeps HubertModel's random init here (sylber.py:41,46); use the seeded one
            return synthetic_state_dict(0, num_layers=encoding_layer)
        if isinstance(model_ckpt, dict):
            return model_ckpt
        if model_ckpt == "sylber":
            model_ckpt = "sylber.ckpt"
        if not Path(model_ckpt).exists():
            from huggingface_hub import hf_hub_download  # sylber.py:49-50
            model_ckpt = hf_hub_download(repo_id="cheoljun95/sylber", filename=model_ckpt)
        sd = torch.load(model_ckpt, map_location="cpu")
        print("Pre-trained checkpoint loaded")
        return sd

    # -- batching exactly like sylber.py:76-118 ---------------------------------------------------
    def _collect(self, wav_file, wav):
        batch_wavs: List[torch.Tensor] = []
        if wav_file is not None:
            is_batch = isinstance(wav_file, list)
            for f in (wav_file if is_batch else [wav_file]):
                # sylber.py:83-86 on the device: decode, resample to 16 kHz, (x - mean) / unbiased std
                batch_wavs.append(ingest_file(f, self.speech_model.device, normalize=True))
        else:
            assert wav is not None
            is_batch = isinstance(wav, list)
            batch_wavs = wav if is_batch else [wav]
        return batch_wavs, is_batch

    @staticmethod
    def _rows(batch_wavs: Sequence[torch.Tensor]):
        rows, lengths = [], []
        for w in batch_wavs:
            if not torch.is_tensor(w) or w.dim() != 2:
                raise ValueError("each wav must be a [channels, N] tensor (sylber.py:96 reads wav.shape[1])")
            for ch in range(w.shape[0]):              # torch.cat(dim=0) makes every channel a batch row
                rows.append(w[ch])
                lengths.append(int(w.shape[1]))
        return rows, lengths

    def encode_batch(self, batch_wavs: Sequence[torch.Tensor]):
        """Pads to the batch max (sylber.py:93-118) and runs the HIP forward.  Returns the device
        hidden states [B,T,768] (full padded T, like the reference) and the per-row lengths."""
        tr = self.__dict__.get("_trace")
        mark = (lambda name: tr.append((name, time.perf_counter()))) if tr is not None else (lambda name: None)
        rows, lengths = self._rows(batch_wavs)
        lmax = max(lengths)
        dev = self.speech_model.device
        mark("  rows collected")
        if all(not r.is_cuda for r in rows):
            # host inputs: pad on the host into a pinned staging buffer and cross PCIe once (a row-by-row copy loop
            # costs a host round trip per utterance).  Two buffers rotate, each with the event of the H2D copy that last
            # read it: encode_batch returns without synchronising, so the host must not refill a buffer whose copy is
            # still queued behind an earlier forward.
            stage, slot = self._stage_buffer((len(rows), lmax))
            # the padding runs through numpy views, NOT torch CPU ops: on a many-core host every small torch op wakes
            # the intra-op thread pool (128 threads on the MI355X boxes), which made one call cost anything from 10 ms
            # to 1.8 s (tools/api_profile.py: 9.4-9.9 ms with one thread, 9.8-188 ms with the default pool)
            stage_np = stage.numpy()
            mark("  staging buffer free")
            batch = torch.empty(len(rows), lmax, dtype=torch.float32, device=dev)
            mark("  device batch allocated")

            # round 4: the 20 MB host copy of a 32 x 10 s batch is 0.47 ms on one thread, 0.26 ms on two, slower again on four or eight
            # (probed on the 256-cpu boxes).  Row groups are padded by a small
            # private thread pool (numpy's copy releases the GIL) and each group crosses PCIe as soon as it is padded, so the
            # H2D of group g runs under the padding of group g + 1
            nrow = len(rows)
            # round 6: twice as many groups as threads -- with one group per thread both groups finish together and the copies only
            # START when the padding is over (tools/api_timeline.py: H2D done 1.25 ms into the call against 0.26 + 0.37 of work)
            ngrp = min(self._fill_groups, max(1, nrow // 4)) if nrow * lmax >= (1 << 20) else 1
            if ngrp <= 1:
                _pad_rows(stage_np, rows, lengths, 0, nrow)
                batch.copy_(stage, non_blocking=True)
            else:
                bounds = [(g * nrow // ngrp, (g + 1) * nrow // ngrp) for g in range(ngrp)]
                futs = [self._fill_pool().submit(_pad_rows, stage_np, rows, lengths, lo, hi) for lo, hi in bounds]
                for (lo, hi), f in zip(bounds, futs):
                    f.result()
                    batch[lo:hi].copy_(stage[lo:hi], non_blocking=True)
            slot["event"].record(torch.cuda.current_stream(dev))
            mark("  padded, H2D issued")
            gtr = self.__dict__.get("_gpu_trace")
            if gtr is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(torch.cuda.current_stream(dev))
                gtr.append(("H2D done", ev))
        else:
            batch = torch.zeros(len(rows), lmax, dtype=torch.float32, device=dev)
            for i, r in enumerate(rows):
                batch[i, : lengths[i]] = r.to(dev, torch.float32, non_blocking=True)
        hidden = self.speech_model.forward(batch, lengths)
        return hidden, lengths

    def _encode_packed(self, batch_wavs: Sequence[torch.Tensor]):
        """packed=True's encode_batch: every clip staged at its slot (``packed_layout``), not into rows of the longest clip, and one
        packed forward.  Returns the device hidden states [offsets[-1], 768], the clips' sample counts, offsets and frame counts."""
        rows, lengths = self._rows(batch_wavs)
        sm = self.speech_model
        sm._check_packed("Segmenter(packed=True)")
        offsets, frames = packed_layout(lengths)
        n = SLOT_SAMPLES * int(offsets[-1])
        dev = sm.device
        if all(not r.is_cuda for r in rows):
            # host inputs: staged in the pinned buffer and uploaded by row groups, as encode_batch does
            stage, slot = self._stage_buffer((n,))
            stage_np = stage.numpy()
            batch = torch.empty(n, dtype=torch.float32, device=dev)
            nrow = len(rows)
            ngrp = min(self._fill_groups, max(1, nrow // 4)) if n >= (1 << 20) else 1
            if ngrp <= 1:
                _stage_packed(stage_np, rows, lengths, offsets, 0, nrow)
                batch.copy_(stage, non_blocking=True)
            else:
                bounds = [(g * nrow // ngrp, (g + 1) * nrow // ngrp) for g in range(ngrp)]
                futs = [self._fill_pool().submit(_stage_packed, stage_np, rows, lengths, offsets, lo, hi) for lo, hi in bounds]
                for (lo, hi), f in zip(bounds, futs):
                    f.result()
                    a, e = SLOT_SAMPLES * int(offsets[lo]), SLOT_SAMPLES * int(offsets[hi])
                    batch[a:e].copy_(stage[a:e], non_blocking=True)
            slot["event"].record(torch.cuda.current_stream(dev))
        else:
            batch = torch.zeros(n, dtype=torch.float32, device=dev)
            for i, r in enumerate(rows):
                a = SLOT_SAMPLES * int(offsets[i])
                batch[a:a + lengths[i]] = r.to(dev, torch.float32, non_blocking=True)
        return sm.forward_packed_raw(batch, lengths, layout=(offsets, frames)), lengths, offsets, frames

    def _fill_pool(self):
        pool = self.__dict__.get("_fill_executor")
        if pool is None:
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(max_workers=self._fill_threads, thread_name_prefix="sylber-pad")
            self._fill_executor = pool
        return pool

    def _stage_buffer(self, shape):
        """next of two grow-only pinned H2D staging buffers; waits (host side) for the copy that last read it"""
        ring = self.__dict__.setdefault("_stage_ring", [{"buf": None, "event": None}, {"buf": None, "event": None}])
        k = self.__dict__.get("_stage_next", 0)
        self._stage_next = (k + 1) % len(ring)
        slot = ring[k]
        n = 1
        for d in shape:
            n *= int(d)
        if slot["event"] is not None:
            slot["event"].synchronize()
        else:
            slot["event"] = torch.cuda.Event()
        if slot["buf"] is None or slot["buf"].numel() < n:
            slot["buf"] = torch.empty(max(n, 1), dtype=torch.float32, pin_memory=True)
        return slot["buf"][:n].view(*shape), slot

    def segment(self, input_values=None, features=None, attention_mask=None, mergethreshold=None, normthreshold=None,
                frames=None, **kwargs):
        """Tensor-native sibling of ``__call__`` with the signature of the reference's ``Sylber.segment``
        (sylber/model/sylber.py:208-247): a padded ``[B, N]`` waveform batch (+ 0/1 ``attention_mask``) or
        precomputed ``features [B, T, 768]`` in, ``(features, segments, avg_fts)`` out — ``segments`` a list of
        int64 ``[n, 2]`` arrays, ``avg_fts`` the segment means zero-padded to ``[B, max(n, 1), 768]`` on the
        device (an utterance without segments contributes one zero row, sylber.py:238-241).
        With ``batch_invariant=True`` every row of the waveform branch is segmented over its own frames (from ``attention_mask``) and
        ``features`` past them are zeroed.  ``frames=`` gives the features branch each row's frame count (default: all ``T``)."""
        dev = self.speech_model.device
        nt = self.norm_threshold if normthreshold is None else normthreshold
        mt = self.merge_threshold if mergethreshold is None else mergethreshold
        if features is None:
            features, frames, seg, nseg, feats, nseg_h, seg_h = self.speech_model.segment_batch(input_values, attention_mask, nt, mt,
                                                                                                self.batch_invariant)
            if self.batch_invariant:
                for b, f in enumerate(frames):
                    features[b, f:] = 0.0
        else:
            features = features.to(dev, torch.float32).contiguous()
            seg, nseg, feats = self.speech_model.segment(features, nt, mt, frames=frames)
            nseg_h, seg_h = _tables_to_host(seg, nseg)
        nmax = seg_h.shape[1]
        keep = torch.arange(nmax, device=dev)[None, :] < nseg[:, None]
        avg_fts = torch.where(keep[:, :, None], feats[:, :nmax], torch.zeros((), device=dev))
        return features, _segment_list(seg_h, nseg_h), avg_fts

    def __call__(self, wav_file=None, wav=None, in_second=True):
        tr = self.__dict__.get("_trace")                     # tools/api_timeline.py: list of (label, host time) marks
        mark = (lambda name: tr.append((name, time.perf_counter()))) if tr is not None else (lambda name: None)
        gtr = self.__dict__.get("_gpu_trace")                # tools/api_timeline.py: list of (label, timing event) recorded on the streams involved
        def gmark(name, stream=None):
            if gtr is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(stream if stream is not None else torch.cuda.current_stream(self.speech_model.device))
                gtr.append((name, ev))
        mark("enter")
        gmark("enter")
        batch_wavs, is_batch = self._collect(wav_file, wav)
        offsets = None
        if self.packed:
            hidden, lengths, offsets, frames = self._encode_packed(batch_wavs)
        else:
            hidden, lengths = self.encode_batch(batch_wavs)
            frames = self.speech_model.frame_counts(lengths) if self.batch_invariant else None
        gmark("forward done")
        mark("padded, H2D and forward issued")
        # D2H (sylber.py:122-138's .cpu().numpy()) into ONE leased page-locked block (PinnedOutputPool: persistent blocks, no
        # page-locking per call); the numpy results are views of that block -- no second host copy of the 49 MB of hidden
        # states per 32 x 10 s batch -- and the block goes back to the pool when the caller drops them.
        # Round 4: the block is leased BEFORE the segmenter runs, sized for the largest segment-slot count seen so far, so
        # that the hidden states (the bulk: 0.87 ms over PCIe) leave on a copy stream WHILE boundary detection runs
        # (0.24 ms + the host's wait for the counts); a batch with more segments than that gets a second block for its
        # tables (rare, and the sizes repeat from then on).
        dev = hidden.device
        cur = torch.cuda.current_stream(dev)
        if offsets is not None:                              # packed: only the clips' own frames leave the device
            B, T, D = len(lengths), int(frames.max()), hidden.shape[1]
            lay = _BlockLayout(B, T, D, min(T, self._kcap_seen), self._want_hidden, self._want_feats, frames=frames)
        else:
            B, T, D = hidden.shape
            lay = _BlockLayout(B, T, D, min(T, self._kcap_seen), self._want_hidden, self._want_feats)
        owner, blk, handed = self._out_block(lay.nbytes, "call")
        copy_s = self.__dict__.get("_copy_stream")
        if copy_s is None or copy_s.device != dev:
            copy_s = self._copy_stream = torch.cuda.Stream(device=dev)
        src = hidden
        if offsets is not None and lay.with_hidden:         # packed: the clips' own rows gathered back to back, then one copy
            src = self.speech_model.gather_packed(hidden, lengths, layout=(offsets, frames))
        fwd_done = self.__dict__.setdefault("_ev_fwd", torch.cuda.Event())
        fwd_done.record(cur)
        if lay.with_hidden:
            with torch.cuda.stream(copy_s):
                copy_s.wait_event(fwd_done)
                lay.hidden(blk).copy_(src, non_blocking=True)
                gmark("hidden states D2H done", copy_s)
            src.record_stream(copy_s)
        if offsets is not None:
            seg, nseg, feats = self.speech_model.segment_packed(hidden, lengths, self.norm_threshold, self.merge_threshold,
                                                                with_features=lay.with_feats, layout=(offsets, frames))
        else:
            seg, nseg, feats = self.speech_model.segment(hidden, self.norm_threshold, self.merge_threshold, with_features=lay.with_feats,
                                                         frames=frames)
        gmark("boundary detection done")
        lay.counts(blk).copy_(nseg, non_blocking=True)
        counted = self.__dict__.setdefault("_ev_counts", torch.cuda.Event())
        counted.record(cur)
        mark("lease, segmenter issued")
        counted.synchronize()                                # the counts are on the host
        mark("counts on the host (forward + boundary detection done)")
        nseg_h = lay.counts(owner).copy()
        k = max(int(nseg_h.max()), 1)
        self._note_segments(k)
        if k > lay.kcap:                                     # more segments than the recent batches had: the tables get their own block
            seg_h, feats_h = _fetch_tables(seg, feats, k)
        else:
            seg_d, feat_d = lay.tables(blk, k)
            seg_d.copy_(seg[:, :k], non_blocking=True)
            if feat_d is not None:
                feat_d.copy_(feats[:, :k], non_blocking=True)
            seg_h, feats_h = lay.tables(owner, k)
        gmark("tables D2H done")
        cur.wait_stream(copy_s)
        cur.synchronize()
        mark("all D2H done")
        if offsets is not None:
            outputs = _result_dicts(nseg_h, seg_h, feats_h, lay.clip_hidden(owner), None, in_second, handed)
        else:
            outputs = _result_dicts(nseg_h, seg_h, feats_h, lay.hidden(owner), frames, in_second, handed)
        mark("dicts built")
        return outputs if is_batch else outputs[0]

    # -- a stream of batches: the PCIe-inclusive path at (nearly) the resident rate -----------------------
    def stream(self, batches, in_second=True):
        """Generator over an iterable of batches (each what ``__call__`` takes as ``wav=``: a list of host ``[channels, N]`` tensors).
        Yields, in order, exactly what ``self(wav=batch, in_second=in_second)`` returns for each of them (same bits: the same
        kernels on the same data) -- but a synchronous call spends ~2.5 of its ~7.6 ms (32 x 10 s) outside the GPU's forward
        (padding + H2D in front, D2H + slicing behind), and here those run under the NEIGHBOURING batches' forwards: batch
        i + 1 is padded and uploaded on a copy stream while batch i computes, batch i's results leave on a second copy stream
        while batch i + 1 computes, and the host slices batch i - 1 meanwhile.  The reference has no counterpart (its
        ``__call__`` is one synchronous batch, sylber.py:76-138); a corpus loop over it is what this replaces."""
        it = iter(batches)
        dev = self.speech_model.device
        cur = torch.cuda.current_stream(dev)
        st = self.__dict__.get("_stream_streams")
        if st is None or st[0].device != dev:
            from .streams import concurrent_streams
            st = self._stream_streams = concurrent_streams(2, dev, avoid=[cur])        # H2D, D2H
        h2d, d2h = st
        want_h, want_f = self._want_hidden, self._want_feats
        counter = {"in": 0}
        NSET = 3                                              # device buffer sets = batches issued ahead + 1

        def ring_set(j):
            ring = self.__dict__.setdefault("_stream_dev", [None] * 8)
            if ring[j] is None:
                ring[j] = {"in_free": None, "out_free": None}
            return ring[j]

        def flat(d, key, numel, dtype):
            buf = d.get(key)
            if buf is None or buf.numel() < numel or buf.device != dev:
                if buf is not None:
                    torch.cuda.synchronize(dev)               # (grow-only: a larger batch shape than any before)
                buf = d[key] = torch.empty(int(numel * 1.25) + 64, dtype=dtype, device=dev)
            return buf[:numel]

        def issue_input(batch_wavs):
            rows, lengths = self._rows(batch_wavs if isinstance(batch_wavs, (list, tuple)) else [batch_wavs])
            if any(r.is_cuda for r in rows):
                raise ValueError("Segmenter.stream takes host tensors (device batches have nothing to overlap: use __call__)")
            lmax = max(lengths)
            n = len(rows)
            offsets = frames = None
            if self.packed:                                   # each clip at its slot, zeros to the slot's end
                self.speech_model._check_packed("Segmenter.stream(packed=True)")
                offsets, frames = packed_layout(lengths)
                stage, slot = self._stage_buffer((SLOT_SAMPLES * int(offsets[-1]),))
                fill, fargs = _stage_packed, (lengths, offsets)
            else:
                stage, slot = self._stage_buffer((len(rows), lmax))
                fill, fargs = _pad_rows, (lengths,)
            stage_np = stage.numpy()
            if self._fill_threads > 1 and n >= 16:
                fut = self._fill_pool().submit(fill, stage_np, rows, *fargs, 0, n // 2)
                fill(stage_np, rows, *fargs, n // 2, n)
                fut.result()
            else:
                fill(stage_np, rows, *fargs, 0, n)
            tr = self.__dict__.get("_trace")
            if tr is not None:
                tr.append(("padded", time.perf_counter()))
            # device buffers come from a ring of three grow-only sets with explicit events, not from the caching allocator: blocks
            # handed between streams with record_stream come back late, and the hipMalloc that then happens every third batch
            # synchronises the device (measured: GPU gaps 5.3 / 5.3 / 6.9 ms, tools/api_stream_timeline.py)
            d = ring_set(counter["in"] % NSET)
            counter["in"] += 1
            with torch.cuda.stream(h2d):
                if d["in_free"] is not None:
                    h2d.wait_event(d["in_free"])
                batch = flat(d, "in", stage.numel(), torch.float32).view(stage.shape)
                batch.copy_(stage, non_blocking=True)
                slot["event"].record(h2d)
                ev = torch.cuda.Event()
                ev.record(h2d)
            return {"batch": batch, "lengths": lengths, "uploaded": ev, "single": not isinstance(batch_wavs, (list, tuple)), "set": d,
                    "offsets": offsets, "pframes": frames}

        def issue_compute(t, slot_id):
            batch, lengths, d = t["batch"], t["lengths"], t["set"]
            cur.wait_event(t["uploaded"])
            if d["out_free"] is not None:
                cur.wait_event(d["out_free"])             # the copies of the batch that last used this set have left
            offsets = t["offsets"]
            if offsets is not None:                           # packed: B clips in offsets[-1] frames, tables of max(frames) slots
                B_, T_, P_ = len(lengths), int(t["pframes"].max()), int(offsets[-1])
            else:
                B_, T_ = batch.shape[0], self.speech_model.num_frames(batch.shape[1])
            # forward + boundary detection run on `cur`, the stream that was current when the generator STARTED, whatever the
            # caller's current stream is at this resumption: `done` below is recorded on the stream the work was issued to
            with torch.cuda.stream(cur):
                out = (flat(d, "seg", B_ * T_ * 2, torch.int64).view(B_, T_, 2), flat(d, "nseg", B_, torch.int32),
                       flat(d, "feat", B_ * T_ * 768, torch.float32).view(B_, T_, 768) if want_f else None)
                if offsets is not None:
                    frames = t["pframes"]
                    hidden = self.speech_model.forward_packed_raw(batch, lengths, out=flat(d, "hid", P_ * 768, torch.float32).view(P_, 768),
                                                                  layout=(offsets, frames))
                    seg, nseg, feats = self.speech_model.segment_packed(hidden, lengths, self.norm_threshold, self.merge_threshold, out=out,
                                                                        layout=(offsets, frames))
                    if want_h:                        # the clips' own rows back to back: one D2H copy below
                        nh = int(frames.sum())
                        hidden = self.speech_model.gather_packed(hidden, lengths, out=flat(d, "cmp", nh * 768, torch.float32).view(nh, 768),
                                                                 layout=(offsets, frames))
                else:
                    hidden = self.speech_model.forward(batch, lengths, out=flat(d, "hid", B_ * T_ * 768, torch.float32).view(B_, T_, 768))
                    frames = self.speech_model.frame_counts(lengths) if self.batch_invariant else None
                    seg, nseg, feats = self.speech_model.segment(hidden, self.norm_threshold, self.merge_threshold, out=out, frames=frames)
            tr = self.__dict__.get("_trace")                  # tools/api_stream_timeline.py: (label, host time[, event]) marks
            done = torch.cuda.Event(enable_timing=tr is not None)
            done.record(cur)
            if tr is not None:
                tr.append(("compute issued", time.perf_counter(), done))
            if offsets is not None:
                B, T, D = B_, T_, 768
                lay = _BlockLayout(B, T, D, min(T, self._kcap_seen), want_h, want_f, frames=frames)
            else:
                B, T, D = hidden.shape
                lay = _BlockLayout(B, T, D, min(T, self._kcap_seen), want_h, want_f)
            # (pageable mode / pool exhausted: one private bounce block per in-flight slot, three)
            owner, blk, handed = self._out_block(lay.nbytes, slot_id)
            with torch.cuda.stream(d2h):
                d2h.wait_event(done)
                if want_h:
                    lay.hidden(blk).copy_(hidden, non_blocking=True)
                lay.counts(blk).copy_(nseg, non_blocking=True)
                seg_d, feat_d = lay.tables(blk)
                seg_d.copy_(seg[:, :lay.kcap], non_blocking=True)
                if want_f:
                    feat_d.copy_(feats[:, :lay.kcap], non_blocking=True)
                out_ev = torch.cuda.Event()
                out_ev.record(d2h)
            d["in_free"], d["out_free"] = done, out_ev
            t.update(dict(layout=lay, owner=owner, handed=handed, out_ev=out_ev, dev=(seg, feats), frames=frames))
            t.pop("batch")
            return t

        def finish(t):
            tr = self.__dict__.get("_trace")
            if tr is not None:
                tr.append(("finish enter", time.perf_counter()))
            t["out_ev"].synchronize()
            if tr is not None:
                tr.append(("results on the host", time.perf_counter()))
            lay, owner = t["layout"], t["owner"]
            nseg_h = lay.counts(owner).copy()
            k = max(int(nseg_h.max()), 1)
            self._note_segments(k)
            seg, feats = t.pop("dev")
            if k > lay.kcap:                              # more segments than the recent batches had: fetch the tables again (rare)
                seg_h, feats_h = _fetch_tables(seg, feats, k)
                torch.cuda.current_stream(dev).synchronize()
            else:
                seg_h, feats_h = lay.tables(owner)
            if lay.frames is not None:
                outputs = _result_dicts(nseg_h, seg_h, feats_h, lay.clip_hidden(owner), None, in_second, t["handed"])
            else:
                outputs = _result_dicts(nseg_h, seg_h, feats_h, lay.hidden(owner), t["frames"], in_second, t["handed"])
            return outputs[0] if t["single"] else outputs

        try:
            first = next(it)
        except StopIteration:
            return
        # two batches are issued ahead of the one being handed out: the D2H of batch i - 1 takes most of batch i's forward (the
        # copies share the chip with 160-KiB-LDS GEMM workgroups), so waiting for it before ISSUING batch i + 1 left the GPU idle
        # now and then (tools/api_stream_timeline.py)
        # the three batches in flight hold a leased block each: they must not eat the consumer's `max_pinned_batches` budget, or every
        # third batch falls back to a pageable copy of its 49 MB of hidden states (a 5 ms host stall, seen as a 7 ms GPU gap)
        budget = self.out_pool.max_leased
        self.out_pool.max_leased = budget + NSET
        pending = []
        # (round 6) the loop makes a few hundred container objects per batch; the full garbage collection they trigger every few batches walks the
        # whole heap of the process (torch, numpy, ...) and stops this thread for 40-120 ms while the GPU drains.  gc.freeze() takes the long-lived
        # heap out of the collector's sight for the duration of the stream (profiles/r06_exchange.md)
        import gc as _gc
        frozen = bool(self.__dict__.get("_freeze_gc", True)) and _gc.isenabled()
        if frozen:
            _gc.freeze()                                                 # (no collect() first: a full collection of this heap is the 40-120 ms this avoids)
        try:
            nxt = issue_input(first)
            i = 0
            while nxt is not None:
                pending.append(issue_compute(nxt, i % NSET))
                try:
                    nxt = issue_input(next(it))           # padded + uploaded under the forward just issued
                except StopIteration:
                    nxt = None
                if len(pending) > NSET - 1:
                    yield finish(pending.pop(0))
                i += 1
            while pending:
                yield finish(pending.pop(0))
        finally:
            # an early exit (consumer stopped, or an exception): the batches still in flight own leased page-locked blocks that
            # the D2H stream may still be writing.  Their owners die with `pending`, the finalizers hand the blocks back, and the next
            # lease could write the same block from another stream -- so wait for those copies first
            for t in pending:
                ev = t.get("out_ev")
                if ev is not None:
                    ev.synchronize()
            pending.clear()
            if frozen:
                _gc.unfreeze()
            self.out_pool.max_leased = budget
            self.out_pool.trim()

    def _note_segments(self, k: int) -> None:
        """size the next leased block from the RECENT per-batch maximum (rounded up to 64, floor 128), not from an all-time one:
        one long-clip batch with many segments must not double every later block for good"""
        self._kcap_recent.append(int(k))
        self._kcap_seen = max(128, (max(self._kcap_recent) + 63) & ~63)

    def _out_block(self, nbytes: int, slot):
        """-> (numpy owner, block tensor, handed): a leased pool block in "pinned" mode while the pool has one to give (handed to the
        caller with the results), else private scratch block ``slot``, reused by the next batch with that slot (results are copied out)"""
        lease = self.out_pool.lease(nbytes) if self.output_memory == "pinned" else None
        if lease is not None:
            return lease[0], lease[1], True
        scratch = self.__dict__.setdefault("_scratch_blocks", {})
        blk = scratch.get(slot)
        if blk is None or blk.numel() < nbytes:
            blk = scratch[slot] = _pinned((nbytes + (1 << 20) - 1) >> 20 << 20)
        return blk.numpy(), blk, False
