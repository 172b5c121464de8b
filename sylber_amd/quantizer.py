"""Host mirror of upstream's learned tokenizer, sylber/model/quantizer.py: ``FFEncoder`` (:15-31), ``_unit_norm`` /
``_unit_norm_sep`` (:33-44), ``load_quantizer`` (:47-77) and ``Quantizer`` (:182-257), eval only, running through the C-ABI of
csrc/downstream.hip (``sylber_lq_norm``, ``sylber_ffenc``, ``sylber_rvq_*``) in exact fp32.

The two ``GroupedResidualVQ`` stacks come from ``vector_quantize_pytorch``; their eval semantics are restated here for one group of
Euclidean codebooks: ``r = x``, and per stage ``i = argmin_k ||r - E[k]||`` (ties to the smallest k), ``z += E[i]``, ``r -= E[i]``.
Everything else of that library (cosine codebooks, projections, several groups or heads, stochastic sampling) is refused by name.

Deviations from upstream, both deliberate: ``load_quantizer(config)`` without weights raises (upstream would build random ones), and
``decode`` clamps ids >= K to K - 1 (upstream would index out of range)."""
from __future__ import annotations

import ctypes
import os
from typing import Dict

import numpy as np
import torch

from . import _lib

ENCODER_KEYS = {"input_dim", "output_dim", "hidden_dims", "dropout"}
# GroupedResidualVQ arguments: the ones the restated semantics need, the ones accepted with one value only, the training-only ones
VQ_KEYS = {"dim", "codebook_size", "num_quantizers"}
VQ_FIXED = {"groups": 1, "heads": 1, "use_cosine_sim": False, "shared_codebook": False, "stochastic_sample_codes": False,
            "accept_image_fmap": False}
VQ_TRAINING = {"decay", "commitment_weight", "kmeans_init", "kmeans_iters", "threshold_ema_dead_code", "sample_codebook_temp",
               "learnable_codebook", "ema_update"}
VQ_TRAINING_PREFIXES = ("quantize_dropout", "orthogonal_reg_")
# buffers of the codebook modules that eval does not read
VQ_IGNORED_BUFFERS = ("initted", "cluster_size", "embed_avg")


def _round(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _check_vq(name: str, cfg, dim: int) -> Dict[str, int]:
    if not isinstance(cfg, dict):
        raise ValueError("%s must be a dict, got %r" % (name, type(cfg).__name__))
    for k, v in cfg.items():
        if k in VQ_KEYS or k in VQ_TRAINING or k.startswith(VQ_TRAINING_PREFIXES):
            continue
        if k == "codebook_dim":
            if v is not None and int(v) != int(cfg.get("dim", -1)):
                raise ValueError("%s['codebook_dim'] = %r: only codebook_dim == dim (no projection) is supported" % (name, v))
            continue
        if k in VQ_FIXED:
            if v != VQ_FIXED[k]:
                raise ValueError("%s[%r] = %r is not supported: only %r" % (name, k, v, VQ_FIXED[k]))
            continue
        raise ValueError("%s has the unsupported key %r" % (name, k))
    for k in sorted(VQ_KEYS):
        if k not in cfg:
            raise ValueError("%s is missing %r" % (name, k))
    out = {k: int(cfg[k]) for k in VQ_KEYS}
    if min(out.values()) < 1:
        raise ValueError("%s: dim, codebook_size and num_quantizers must be >= 1, got %s" % (name, out))
    if out["dim"] != dim:
        raise ValueError("%s['dim'] = %d, but the encoder hands this stack %d columns" % (name, out["dim"], dim))
    return out


def check_quantizer_config(encoder_configs, art_vq_configs, pitch_vq_configs, pitch_emb_dim=8) -> dict:
    """The pure-host validation of ``Quantizer``'s arguments.  Returns the geometry ``{"input_dim", "hidden_dims", "output_dim",
    "A", "p", "art": {dim, codebook_size, num_quantizers}, "pitch": {...}}``; anything outside the supported surface is a
    ``ValueError`` naming the key."""
    if not isinstance(encoder_configs, dict):
        raise ValueError("encoder_configs must be a dict")
    for k in encoder_configs:
        if k not in ENCODER_KEYS:
            raise ValueError("encoder_configs has the unsupported key %r" % (k,))
    for k in ("input_dim", "output_dim", "hidden_dims"):
        if k not in encoder_configs:
            raise ValueError("encoder_configs is missing %r" % (k,))
    ind, outd = int(encoder_configs["input_dim"]), int(encoder_configs["output_dim"])
    hidden = [int(h) for h in encoder_configs["hidden_dims"]]
    if ind < 1 or outd < 1 or any(h < 1 for h in hidden):
        raise ValueError("encoder_configs: input_dim, output_dim and hidden_dims must be >= 1")
    p = int(pitch_emb_dim)
    if p < 1:
        raise ValueError("pitch_emb_dim = %d: must be >= 1 (upstream's [..., :-0] would leave the art stack nothing)" % p)
    A = outd - p
    if A < 1:
        raise ValueError("pitch_emb_dim = %d leaves no art columns of output_dim = %d" % (p, outd))
    return {"input_dim": ind, "hidden_dims": hidden, "output_dim": outd, "A": A, "p": p,
            "art": _check_vq("art_vq_configs", art_vq_configs, A), "pitch": _check_vq("pitch_vq_configs", pitch_vq_configs, p)}


def _cpu32(t) -> torch.Tensor:
    return torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).detach().to("cpu", torch.float32)


def _vp(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _encoder_layers(geom) -> list:
    """(state-dict prefix, out, in) of every Linear of FFEncoder, in upstream's order (quantizer.py:19-28)"""
    widths = [geom["input_dim"]] + geom["hidden_dims"]
    layers = []
    for i, h in enumerate(geom["hidden_dims"]):
        layers += [("encoder.mlp.%d" % (2 * i), h, widths[i]), ("encoder.mlp.%d.0" % (2 * i + 1), h, h),
                   ("encoder.mlp.%d.3" % (2 * i + 1), h, h)]
    return layers + [("encoder.mlp.%d" % (2 * len(geom["hidden_dims"])), geom["output_dim"], widths[-1])]


def padded_host_weights(geom, sd: Dict[str, torch.Tensor]):
    """upstream's ``load_state_dict(sd, strict=True)`` for the geometry ``check_quantizer_config`` returns, on the host: a missing
    tensor is a ``KeyError`` naming it, and so is an unexpected key (the codebooks' ``initted`` / ``cluster_size`` / ``embed_avg``
    buffers are read by training only and ignored); a tensor of the wrong shape is a ``ValueError``.  A codebook may be
    ``[1, K, d]`` (upstream's buffer) or ``[K, d]``.
    Returns ``(encoder, books)``: the encoder's (W, b) pairs in launch order, zero-padded to multiples of 16, and
    ``{"art_vq" / "pitch_vq": (codebooks [Q, Kp, dp], K, d)}`` with K padded to a multiple of 4 and d to 16, the padding zero."""
    layers = _encoder_layers(geom)
    stacks = {"art_vq": geom["art"], "pitch_vq": geom["pitch"]}
    expected = set()
    for name, _, _ in layers:
        expected |= {name + ".weight", name + ".bias"}
    for st, vc in stacks.items():
        expected |= {"%s.rvqs.0.layers.%d._codebook.embed" % (st, q) for q in range(vc["num_quantizers"])}
    for k in sd:
        if k in expected:
            continue
        if k.startswith(("art_vq.", "pitch_vq.")) and k.rsplit(".", 1)[-1] in VQ_IGNORED_BUFFERS:
            continue
        raise KeyError("unexpected key in the Quantizer state_dict: %r" % (k,))
    for k in sorted(expected):
        if k not in sd:
            raise KeyError("the Quantizer state_dict is missing %r" % (k,))
    enc = []
    for name, out_f, in_f in layers:
        w, b = _cpu32(sd[name + ".weight"]), _cpu32(sd[name + ".bias"])
        if tuple(w.shape) != (out_f, in_f) or tuple(b.shape) != (out_f,):
            raise ValueError("%s: weight %s / bias %s, expected %s / %s" % (name, tuple(w.shape), tuple(b.shape), (out_f, in_f), (out_f,)))
        wp = torch.zeros(_round(out_f, 16), _round(in_f, 16), dtype=torch.float32)
        wp[:out_f, :in_f] = w
        bp = torch.zeros(_round(out_f, 16), dtype=torch.float32)
        bp[:out_f] = b
        enc += [wp, bp]
    books = {}
    for st, vc in stacks.items():
        Q, K, d = vc["num_quantizers"], vc["codebook_size"], vc["dim"]
        cb = torch.zeros(Q, _round(K, 4), _round(d, 16), dtype=torch.float32)
        for q in range(Q):
            key = "%s.rvqs.0.layers.%d._codebook.embed" % (st, q)
            e = _cpu32(sd[key])
            if e.dim() == 3 and e.shape[0] == 1:
                e = e[0]
            if tuple(e.shape) != (K, d):
                raise ValueError("%s has shape %s, expected [1, %d, %d] or [%d, %d]" % (key, tuple(sd[key].shape), K, d, K, d))
            cb[q, :K, :d] = e
        books[st] = (cb, K, d)
    return enc, books


class Quantizer:
    """``Quantizer(encoder_configs, art_vq_configs, pitch_vq_configs, unit_norm_encoder_input=True, unit_norm_encoder_output=True,
    keep_blank_zero=True, pitch_emb_dim=8, separate_norm=True)`` of quantizer.py:182, eval.  ``state_dict``: upstream's
    ``Quantizer.state_dict()`` keys (``encoder.mlp.*``, ``{art,pitch}_vq.rvqs.0.layers.{q}._codebook.embed``); without it the weights
    must come through ``load_state_dict`` before the first call."""

    def __init__(self, encoder_configs, art_vq_configs, pitch_vq_configs, unit_norm_encoder_input=True, unit_norm_encoder_output=True,
                 keep_blank_zero=True, pitch_emb_dim=8, separate_norm=True, state_dict=None, device="cuda"):
        self.config = check_quantizer_config(encoder_configs, art_vq_configs, pitch_vq_configs, pitch_emb_dim)
        self.lib = _lib.load()
        if not torch.cuda.is_available() or "cuda" not in str(device):
            raise _lib.SylberHipError("sylber_amd.Quantizer runs on the MI355X only (device=%r); the HIP path has no CPU fallback" % (device,))
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.unit_norm_encoder_input = bool(unit_norm_encoder_input)
        self.unit_norm_encoder_output = bool(unit_norm_encoder_output)
        self.keep_blank_zero = bool(keep_blank_zero)
        self.separate_norm = bool(separate_norm)
        c = self.config
        self.input_dim, self.output_dim = c["input_dim"], c["output_dim"]
        self.pitch_emb_dim, self.art_emb_dim = c["p"], c["A"]
        self.art_codebook_num, self.pitch_codebook_num = c["art"]["num_quantizers"], c["pitch"]["num_quantizers"]
        self._loaded = False
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- weights ------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """upstream's ``load_state_dict(sd, strict=True)`` through ``padded_host_weights``; the padded weights move to the device
        once and every codebook row's squared norm is computed there once"""
        enc, books = padded_host_weights(self.config, sd)
        dev = self.device
        self._enc = [t.to(dev).contiguous() for t in enc]
        widths = [self.config["input_dim"]] + self.config["hidden_dims"] + [self.config["output_dim"]]
        self._dims = (ctypes.c_int32 * len(widths))(*[_round(d, 16) for d in widths])
        self._wptrs = (ctypes.c_void_p * len(self._enc))(*[t.data_ptr() for t in self._enc])
        self._books = {}
        for st, (cb, K, d) in books.items():
            Q, Kp = cb.shape[0], cb.shape[1]
            cb = cb.to(dev).contiguous()
            sq = torch.empty(Q, Kp, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(self.lib.sylber_rvq_prepare(_vp(cb), Q, K, d, _vp(sq), self._stream()), "sylber_rvq_prepare")
            self._books[st] = (cb, sq, Q, K, d)
        self._loaded = True

    @property
    def codebooks(self):
        """the unpadded codebooks ``{"art_vq": [Qa, K, A], "pitch_vq": [Qp, K, p]}`` (device tensors)"""
        return {st: cb[:, :K, :d] for st, (cb, _, _, K, d) in self._books.items()}

    # ---- compute ------------------------------------------------------------------------------------------------------------
    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, token):
        if not self._loaded:
            raise RuntimeError("Quantizer has no weights: pass state_dict= or call load_state_dict first")
        t = token if torch.is_tensor(token) else torch.from_numpy(np.asarray(token))
        if t.dim() < 1 or t.shape[-1] != self.input_dim:
            raise ValueError("token must be [..., %d], got %s" % (self.input_dim, tuple(t.shape)))
        lead = tuple(t.shape[:-1])
        return lead, t.reshape(-1, self.input_dim).to(self.device, torch.float32).contiguous()

    def _norm(self, x, ldx, n, D, y, ldy, Dy, normalize, split=0, blank=None):
        c = self.lib.sylber_lq_norm(_vp(x), ldx, n, D, split, 1 if normalize else 0, _vp(blank) if blank is not None else None,
                                    self.input_dim, self.input_dim, _vp(y), ldy, Dy, self._stream())
        _lib.check(c, "sylber_lq_norm")

    def _split(self) -> int:
        return self.art_emb_dim if self.separate_norm else 0

    def _run(self, x: torch.Tensor, with_z: bool):
        n, O, A = x.shape[0], self.output_dim, self.art_emb_dim
        dev = self.device
        Qa, Qp = self.art_codebook_num, self.pitch_codebook_num
        ids = torch.empty(n, Qa + Qp, dtype=torch.int32, device=dev)
        nq = torch.empty(n, O, dtype=torch.float32, device=dev)
        z = torch.empty(n, O, dtype=torch.float32, device=dev) if with_z else None
        d0, dO = self._dims[0], self._dims[len(self._dims) - 1]
        x0 = torch.empty(n, d0, dtype=torch.float32, device=dev)
        enc = torch.empty(n, dO, dtype=torch.float32, device=dev)
        wsz = max(int(self.lib.sylber_ffenc_workspace_floats(n, len(self.config["hidden_dims"]), self._dims)),
                  *[int(self.lib.sylber_rvq_workspace_floats(n, K, d)) for (_, _, _, K, d) in self._books.values()])
        ws = torch.empty(wsz, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            s = self._stream()
            # 1-2: the token, unit-normalised (or copied) into the zero-padded encoder input
            self._norm(x, self.input_dim, n, self.input_dim, x0, d0, d0, self.unit_norm_encoder_input)
            # 3: FFEncoder
            _lib.check(self.lib.sylber_ffenc(_vp(x0), n, len(self.config["hidden_dims"]), self._dims, self._wptrs, _vp(enc), _vp(ws), s),
                       "sylber_ffenc")
            # 4-5: the output norm (art / pitch separately) and the blank rows of the token as given
            self._norm(enc, dO, n, O, nq, O, O, self.unit_norm_encoder_output, self._split(), x if self.keep_blank_zero else None)
            # 6: both residual stacks on column windows of the same rows
            for st, col, icol in (("art_vq", 0, 0), ("pitch_vq", A, Qa)):
                cb, sq, Q, K, d = self._books[st]
                zp = ctypes.c_void_p(z.data_ptr() + 4 * col) if z is not None else None
                _lib.check(self.lib.sylber_rvq_assign(ctypes.c_void_p(nq.data_ptr() + 4 * col), O, n, d, _vp(cb), _vp(sq), Q, K,
                                                      ctypes.c_void_p(ids.data_ptr() + 4 * icol), Qa + Qp, zp, O, _vp(ws), s),
                           "sylber_rvq_assign")
            if z is not None and self.unit_norm_encoder_output:
                self._norm(z, O, n, O, z, O, O, True, self._split())        # 7, in place
        return ids, nq, z

    def get_indices(self, token) -> torch.Tensor:
        """token ``[..., input_dim]`` (tensor on any device, or array) -> int64 ids ``[..., Qa + Qp]`` on the device"""
        lead, x = self._rows(token)
        if x.shape[0] == 0:
            return torch.empty(lead + (self.art_codebook_num + self.pitch_codebook_num,), dtype=torch.int64, device=self.device)
        ids, _, _ = self._run(x, with_z=False)
        return ids.to(torch.int64).reshape(lead + (ids.shape[1],))

    def forward(self, token) -> Dict[str, torch.Tensor]:
        """upstream's ``forward``: ``{"indices", "quantize", "non_quantized", "commitment_loss"}`` (the loss is 0 in eval)"""
        lead, x = self._rows(token)
        O, Qn = self.output_dim, self.art_codebook_num + self.pitch_codebook_num
        if x.shape[0] == 0:
            e = torch.empty(lead + (O,), dtype=torch.float32, device=self.device)
            ids = torch.empty(lead + (Qn,), dtype=torch.int64, device=self.device)
            return {"indices": ids, "quantize": e, "non_quantized": e.clone(), "commitment_loss": torch.zeros((), device=self.device)}
        ids, nq, z = self._run(x, with_z=True)
        return {"indices": ids.to(torch.int64).reshape(lead + (Qn,)), "quantize": z.reshape(lead + (O,)),
                "non_quantized": nq.reshape(lead + (O,)), "commitment_loss": torch.zeros((), device=self.device)}

    __call__ = forward

    def decode(self, indices) -> torch.Tensor:
        """ids ``[..., Qa + Qp]`` -> ``[..., output_dim]``: each stack's codebook rows summed in stage order, concatenated, normalised
        as the encoder output.  Negative ids are clipped to 0 (upstream), ids >= K clamped to K - 1."""
        if not self._loaded:
            raise RuntimeError("Quantizer has no weights: pass state_dict= or call load_state_dict first")
        t = indices if torch.is_tensor(indices) else torch.from_numpy(np.asarray(indices))
        Qa, Qp, O, A = self.art_codebook_num, self.pitch_codebook_num, self.output_dim, self.art_emb_dim
        if t.dim() < 1 or t.shape[-1] != Qa + Qp:
            raise ValueError("indices must be [..., %d], got %s" % (Qa + Qp, tuple(t.shape)))
        lead = tuple(t.shape[:-1])
        ids = t.reshape(-1, Qa + Qp).to(self.device).to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
        n = ids.shape[0]
        z = torch.empty(n, O, dtype=torch.float32, device=self.device)
        if n:
            with torch.cuda.device(self.device):
                for st, col, icol in (("art_vq", 0, 0), ("pitch_vq", A, Qa)):
                    cb, _, Q, K, d = self._books[st]
                    _lib.check(self.lib.sylber_rvq_decode(ctypes.c_void_p(ids.data_ptr() + 4 * icol), Qa + Qp, n, _vp(cb), Q, K, d,
                                                          ctypes.c_void_p(z.data_ptr() + 4 * col), O, self._stream()), "sylber_rvq_decode")
                if self.unit_norm_encoder_output:
                    self._norm(z, O, n, O, z, O, O, True, self._split())
        return z.reshape(lead + (O,))

    def eval(self):
        return self


def _read_config(path: str) -> dict:
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def resolve_quantizer_args(config=None, ckpt=None):
    """the argument forms of ``load_quantizer`` (quantizer.py:47-77) -> ``(config dict, state_dict)``, on the host.
    ``config``: a dict, a YAML path (optionally nested under ``model``) or a ``.ckpt`` path holding ``{"config", "state_dict"}``;
    ``ckpt``: a checkpoint path or an already loaded dict (``{"config", "state_dict"}``, ``{"state_dict"}`` or a bare state dict).
    Weights are required: a config alone is a ``ValueError`` (upstream would build a randomly initialised quantizer)."""
    def load(c):
        return torch.load(c, map_location="cpu", weights_only=True) if not isinstance(c, dict) else c

    state_dict = None
    if config is not None:
        if not isinstance(config, dict):
            config = os.fspath(config)
            if config.endswith(".ckpt"):
                return resolve_quantizer_args(config=None, ckpt=config)
            config = _read_config(config)
        if "model" in config:
            config = config["model"]
        if ckpt is not None:
            obj = load(ckpt)
            state_dict = obj["state_dict"] if "state_dict" in obj else obj
    else:
        if ckpt is None:
            raise ValueError("load_quantizer needs a config, a checkpoint, or both")
        obj = load(ckpt)
        if "config" not in obj or "state_dict" not in obj:
            raise KeyError("a checkpoint passed without a config must hold {'config', 'state_dict'}")
        config, state_dict = obj["config"], obj["state_dict"]
    if state_dict is None:
        raise ValueError("load_quantizer(config) without weights: upstream would build a randomly initialised quantizer; pass ckpt=")
    return dict(config), state_dict


def load_quantizer(config=None, ckpt=None, device="cuda") -> Quantizer:
    """quantizer.py:47-77 with the argument forms of ``resolve_quantizer_args``; returns a ``Quantizer`` on ``device``"""
    config, state_dict = resolve_quantizer_args(config, ckpt)
    return Quantizer(**config, state_dict=state_dict, device=device)
