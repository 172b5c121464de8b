"""Weight schema of the hot path and a deterministic synthetic checkpoint.

The reference loads a flat ``state_dict`` with ``load_state_dict(strict=False)`` into
``transformers.HubertModel`` (sylber/model/sylber.py:41-52).  The real checkpoint (``sylber.ckpt``
on the HF hub, sylber.py:47-50) is not obtainable offline, so benchmarks, tests and golden
vectors use the seeded synthetic checkpoint built here.  Key names and shapes follow
``HubertModel.state_dict()`` for the 9-layer hubert-base geometry.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

CONV_KERNELS = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)
CONV_DIM = 512
HIDDEN = 768
HEADS = 12
FFN = 3072
POS_K = 128
POS_GROUPS = 16
NUM_LAYERS = 9

POS_G_KEYS = ("encoder.pos_conv_embed.conv.parametrizations.weight.original0",
              "encoder.pos_conv_embed.conv.weight_g")
POS_V_KEYS = ("encoder.pos_conv_embed.conv.parametrizations.weight.original1",
              "encoder.pos_conv_embed.conv.weight_v")


def expected_shapes(num_layers: int = NUM_LAYERS) -> Dict[str, tuple]:
    s: Dict[str, tuple] = {"masked_spec_embed": (HIDDEN,)}
    for i, k in enumerate(CONV_KERNELS):
        s[f"feature_extractor.conv_layers.{i}.conv.weight"] = (CONV_DIM, 1 if i == 0 else CONV_DIM, k)
    s["feature_extractor.conv_layers.0.layer_norm.weight"] = (CONV_DIM,)
    s["feature_extractor.conv_layers.0.layer_norm.bias"] = (CONV_DIM,)
    s["feature_projection.layer_norm.weight"] = (CONV_DIM,)
    s["feature_projection.layer_norm.bias"] = (CONV_DIM,)
    s["feature_projection.projection.weight"] = (HIDDEN, CONV_DIM)
    s["feature_projection.projection.bias"] = (HIDDEN,)
    s["encoder.pos_conv_embed.conv.bias"] = (HIDDEN,)
    s[POS_G_KEYS[0]] = (1, 1, POS_K)
    s[POS_V_KEYS[0]] = (HIDDEN, HIDDEN // POS_GROUPS, POS_K)
    s["encoder.layer_norm.weight"] = (HIDDEN,)
    s["encoder.layer_norm.bias"] = (HIDDEN,)
    for l in range(num_layers):
        p = f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"attention.{n}.weight"] = (HIDDEN, HIDDEN)
            s[p + f"attention.{n}.bias"] = (HIDDEN,)
        s[p + "layer_norm.weight"] = (HIDDEN,)
        s[p + "layer_norm.bias"] = (HIDDEN,)
        s[p + "feed_forward.intermediate_dense.weight"] = (FFN, HIDDEN)
        s[p + "feed_forward.intermediate_dense.bias"] = (FFN,)
        s[p + "feed_forward.output_dense.weight"] = (HIDDEN, FFN)
        s[p + "feed_forward.output_dense.bias"] = (HIDDEN,)
        s[p + "final_layer_norm.weight"] = (HIDDEN,)
        s[p + "final_layer_norm.bias"] = (HIDDEN,)
    return s


def synthetic_state_dict(seed: int = 0, num_layers: int = NUM_LAYERS, final_gain: float = 0.038,
                         final_bias: float = 1.0, final_spread: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded fp32 checkpoint with HF-init-like scales.

    Linear ~ N(0, 0.02)... scaled up so that attention and FFN actually move the residual stream
    (pure 0.02 init makes every layer a near-identity, which would hide kernel bugs); convs
    kaiming-normal; LayerNorm/GroupNorm affine drawn around (1, 0).  The LAST layer's
    ``final_layer_norm`` is given a small gain and a fixed bias direction so that frame norms
    straddle the reference's ``norm_threshold=2.6`` and adjacent-frame cosines straddle
    ``merge_threshold=0.8`` (sylber.py:35-36): with unit gain every frame norm is ~27.7 and the
    segmenter would see one all-speech segment.
    """
    g = torch.Generator().manual_seed(seed)

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    sd: Dict[str, torch.Tensor] = {}
    shapes = expected_shapes(num_layers)
    for name, shape in shapes.items():
        if name == "masked_spec_embed":
            sd[name] = torch.rand(*shape, generator=g)
        elif name.endswith("conv.weight") and name.startswith("feature_extractor"):
            fan_in = shape[1] * shape[2]
            sd[name] = randn(*shape, std=math.sqrt(2.0 / fan_in))
        elif "layer_norm.weight" in name:
            sd[name] = 1.0 + randn(*shape, std=0.1)
        elif "layer_norm.bias" in name:
            sd[name] = randn(*shape, std=0.1)
        elif name == POS_G_KEYS[0]:
            sd[name] = 1.0 + 0.25 * torch.rand(*shape, generator=g)
        elif name == POS_V_KEYS[0]:
            sd[name] = randn(*shape, std=math.sqrt(4.0 / (POS_K * HIDDEN)))
        elif name.endswith(".bias"):
            sd[name] = randn(*shape, std=0.02)
        elif name.endswith(".weight"):
            # linear layers: fan-in scaled so activations keep O(1) scale through the stack; the
            # two residual-branch output projections are damped so that 9 random layers do not
            # collapse every frame onto one common direction (adjacent-frame cosine -> 1).
            damp = 0.3 if ("out_proj" in name or "output_dense" in name) else 1.0
            sd[name] = randn(*shape, std=damp / math.sqrt(shape[1]))
        else:
            raise KeyError(name)
    last = f"encoder.layers.{num_layers - 1}.final_layer_norm."
    sd[last + "weight"] = final_gain * torch.exp(final_spread * randn(HIDDEN))
    direction = randn(HIDDEN)
    sd[last + "bias"] = final_bias * direction / direction.norm()
    return sd


def normalize_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Accept both the parametrized (``parametrizations.weight.original{0,1}``) and the legacy
    (``weight_g`` / ``weight_v``) pos-conv names, and an optional ``speech_model.`` prefix."""
    out = {}
    for k, v in sd.items():
        for pre in ("speech_model.", "hubert."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k == POS_G_KEYS[1]:
            k = POS_G_KEYS[0]
        if k == POS_V_KEYS[1]:
            k = POS_V_KEYS[0]
        out[k] = v
    return out


def fold_pos_conv_weight(sd: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Effective positional-conv weight ``g * v / ||v||`` (weight_norm with dim=2: the norm runs over
    dims (0, 1) for every tap; TP:63-80).  Folded once at load time; also accepts a plain
    ``conv.weight`` entry."""
    sd = normalize_keys(sd)
    if POS_G_KEYS[0] in sd:
        g = sd[POS_G_KEYS[0]].float()
        v = sd[POS_V_KEYS[0]].float()
        return (g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()).contiguous()
    return sd["encoder.pos_conv_embed.conv.weight"].float().contiguous()


def synthetic_mlp_state_dict(seed: int = 0, input_dim: int = HIDDEN, output_dim: int = 256,
                             hidden_dims=(512, 512)) -> Dict[str, torch.Tensor]:
    """Seeded weights of the resynthesis conditioner ``MLP`` in the key layout of its ``state_dict()``
    (sylber/model/segment_synthesis.py:35-53: ``mlp.{2i}`` Linear, ``mlp.{2i+1}`` RFF with ``linear1``, ``linear2``,
    ``norm``; last entry the output Linear; sylber_configs/sylber_resynthesis.yaml gives 768 -> [512, 512] -> 256)."""
    g = torch.Generator().manual_seed(10_000 + seed)

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    sd: Dict[str, torch.Tensor] = {}
    d_in = input_dim
    for i, d in enumerate(hidden_dims):
        sd["mlp.%d.weight" % (2 * i)] = randn(d, d_in, std=1.0 / math.sqrt(d_in))
        sd["mlp.%d.bias" % (2 * i)] = randn(d, std=0.1)
        for nm in ("linear1", "linear2"):
            sd["mlp.%d.%s.weight" % (2 * i + 1, nm)] = randn(d, d, std=1.0 / math.sqrt(d))
            sd["mlp.%d.%s.bias" % (2 * i + 1, nm)] = randn(d, std=0.1)
        sd["mlp.%d.norm.weight" % (2 * i + 1)] = 1.0 + randn(d, std=0.1)
        sd["mlp.%d.norm.bias" % (2 * i + 1)] = randn(d, std=0.1)
        d_in = d
    sd["mlp.%d.weight" % (2 * len(hidden_dims))] = randn(output_dim, d_in, std=1.0 / math.sqrt(d_in))
    sd["mlp.%d.bias" % (2 * len(hidden_dims))] = randn(output_dim, std=0.1)
    return sd


# ---- the resynthesis decoder (flow-matching Regressor, sylber_configs/sylber_resynthesis.yaml geometry) ----------------------
CFM_DIM, CFM_DEPTH, CFM_HEADS, CFM_DIM_HEAD = 512, 8, 8, 64
CFM_DIM_IN_PROJ, CFM_DIM_COND_EMB, CFM_DIM_OUT = 64, 256, 14
CFM_REGISTERS, CFM_CONV_K, CFM_FF_MULT = 16, 31, 4
CFM_FF_INNER = int(CFM_DIM * CFM_FF_MULT * 2 / 3)      # 1365 (FeedForward, flowmatching.py)
CFM_TIME_HIDDEN = CFM_DIM * 4                           # 2048
CFM_ROTARY_THETA = 50000


def synthetic_regressor_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded weights of the flow-matching ``Regressor`` (sylber/model/flowmatching.py:474-688) in the key layout of its
    ``state_dict()``, at the sylber_resynthesis.yaml geometry (dim 512, depth 8, 8 x 64 heads, dim_cond_emb 256,
    dim_in_proj 64, 16 register tokens, conv kernel 31, ff_mult 4).  CPU torch generator, so every machine builds the same
    tensors.

    The scaling is chosen to look like a TRAINED decoder rather than the reference's initialisation:
      * residual output projections (attention ``to_out``, FF out) at 0.3 / sqrt(fan_in): each block adds a fraction of the
        residual stream instead of doubling it;
      * q / k ``MultiheadRMSNorm`` gains around 0.3: with the Attend scale of 10 on top of the norm-8 q and k the reference's
        unit gains give attention logits of 370-410, where any 16-bit rounding of the operands changes which key wins (a
        chaotic decoder); at 0.3 the logits stay in the 30s;
      * AdaRMSNorm ``to_gamma`` / ``to_beta`` with nonzero weights and gains around 1, so that the time conditioning is
        exercised (the reference initialises them to the identity, which would leave that path untested);
      * ``to_embed`` bias at std 1 (a residual stream of norm ~20 even where the conditioning is zero): at 0.1, the
        silence-masked and zero-padded frames carry a residual of norm ~3 that the RMSNorms blow up, and the sampler's
        Lipschitz constant there is ~200 -- a 1e-5 change of the input moves the 5-step sample by 0.4 relative RMS, so no
        two implementations (or summation orders) agree.  At std 1 both kinds of frames sit near 0.5-0.7;
      * everything else at 1 / sqrt(fan_in), biases at 0.05-0.1, learned sinusoidal frequencies and register tokens at
        std 1 as in the reference."""
    g = torch.Generator().manual_seed(20_000 + seed)

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    D, TH, FI, HD = CFM_DIM, CFM_TIME_HIDDEN, CFM_FF_INNER, CFM_HEADS * CFM_DIM_HEAD
    sd: Dict[str, torch.Tensor] = {}
    sd["proj_in.weight"] = randn(CFM_DIM_IN_PROJ, CFM_DIM_OUT, std=1.0 / math.sqrt(CFM_DIM_OUT))
    sd["proj_in.bias"] = randn(CFM_DIM_IN_PROJ, std=0.1)
    sd["sinu_pos_emb.0.weights"] = randn(D // 2)
    sd["sinu_pos_emb.1.weight"] = randn(TH, D, std=1.0 / math.sqrt(D))
    sd["sinu_pos_emb.1.bias"] = randn(TH, std=0.1)
    sd["to_cond_emb.weight"] = randn(501, CFM_DIM_COND_EMB)          # unused at inference (cond_emb is passed in)
    sd["to_embed.weight"] = randn(D, 2 * CFM_DIM_IN_PROJ + CFM_DIM_COND_EMB, std=1.0 / math.sqrt(2 * CFM_DIM_IN_PROJ + CFM_DIM_COND_EMB))
    sd["to_embed.bias"] = randn(D, std=1.0)
    sd["null_cond"] = torch.zeros(D)
    sd["conv_embed.dw_conv1d.0.weight"] = randn(D, 1, CFM_CONV_K, std=1.0 / math.sqrt(CFM_CONV_K))
    sd["conv_embed.dw_conv1d.0.bias"] = randn(D, std=0.1)
    sd["transformer.register_tokens"] = randn(CFM_REGISTERS, D)
    sd["transformer.rotary_emb.inv_freq"] = 1.0 / (CFM_ROTARY_THETA ** (torch.arange(0, CFM_DIM_HEAD, 2).float() / CFM_DIM_HEAD))
    for i in range(CFM_DEPTH):
        p = "transformer.layers.%d." % i
        for n in (2, 4):
            sd[p + "%d.to_gamma.weight" % n] = randn(D, TH, std=0.3 / math.sqrt(TH))
            sd[p + "%d.to_gamma.bias" % n] = 1.0 + randn(D, std=0.1)
            sd[p + "%d.to_beta.weight" % n] = randn(D, TH, std=0.1 / math.sqrt(TH))
            sd[p + "%d.to_beta.bias" % n] = randn(D, std=0.05)
        sd[p + "3.q_norm.gamma"] = 0.3 * (1.0 + randn(CFM_HEADS, 1, CFM_DIM_HEAD, std=0.1))
        sd[p + "3.k_norm.gamma"] = 0.3 * (1.0 + randn(CFM_HEADS, 1, CFM_DIM_HEAD, std=0.1))
        sd[p + "3.to_qkv.weight"] = randn(3 * HD, D, std=1.0 / math.sqrt(D))
        sd[p + "3.to_out.weight"] = randn(D, HD, std=0.3 / math.sqrt(HD))
        sd[p + "5.0.weight"] = randn(2 * FI, D, std=1.0 / math.sqrt(D))
        sd[p + "5.0.bias"] = randn(2 * FI, std=0.05)
        sd[p + "5.3.weight"] = randn(D, FI, std=0.3 / math.sqrt(FI))
        sd[p + "5.3.bias"] = randn(D, std=0.05)
    sd["transformer.final_norm.gamma"] = 1.0 + randn(D, std=0.1)
    sd["to_pred.weight"] = randn(CFM_DIM_OUT, D, std=1.0 / math.sqrt(D))
    return sd


# ---- the learned quantizer (sylber/model/quantizer.py:182-257) ------------------------------------------------------------------
def synthetic_quantizer_state_dict(config: dict, seed: int = 0, bias_std: float = 0.01) -> Dict[str, torch.Tensor]:
    """Seeded weights of upstream's ``Quantizer(**config)`` in the key layout of its ``state_dict()``: ``encoder.mlp.*`` and
    ``{art,pitch}_vq.rvqs.0.layers.{q}._codebook.embed`` ``[1, K, d]`` (with the ``initted`` / ``cluster_size`` / ``embed_avg``
    buffers a trained checkpoint carries).  Codebooks that make near-ties rare: stage 0 holds the (normalised, if the config says
    so) encoder outputs of random tokens, computed here in float64; later stages are random rows at a smaller scale each."""
    from .quantizer import _encoder_layers, check_quantizer_config
    geom = check_quantizer_config(config["encoder_configs"], config["art_vq_configs"], config["pitch_vq_configs"],
                                  config.get("pitch_emb_dim", 8))
    g = torch.Generator().manual_seed(20_000 + seed)

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * std

    sd: Dict[str, torch.Tensor] = {}
    layers = []
    for name, out_f, in_f in _encoder_layers(geom):
        w, b = randn(out_f, in_f, std=1.0 / math.sqrt(in_f)), randn(out_f, std=bias_std)
        sd[name + ".weight"], sd[name + ".bias"] = w.float(), b.float()
        layers.append((name, w, b))

    def unit(x):
        return x / torch.sqrt((x ** 2).sum(-1, keepdim=True) + 1e-5)

    A, p = geom["A"], geom["p"]
    Kmax = max(geom["art"]["codebook_size"], geom["pitch"]["codebook_size"])
    x = randn(Kmax, geom["input_dim"])
    if config.get("unit_norm_encoder_input", True):
        x = unit(x)
    for name, w, b in layers:
        x = x @ w.T + b
        if name.endswith(".0"):
            x = torch.relu(x)
    if config.get("unit_norm_encoder_output", True):
        x = torch.cat([unit(x[:, :A]), unit(x[:, A:])], 1) if config.get("separate_norm", True) else unit(x)
    for st, cols in (("art_vq", x[:, :A]), ("pitch_vq", x[:, A:])):
        vc = geom["art" if st == "art_vq" else "pitch"]
        K, d = vc["codebook_size"], vc["dim"]
        scale = float(torch.sqrt((cols[:K] ** 2).sum(-1).mean()))
        for q in range(vc["num_quantizers"]):
            e = cols[:K] + randn(K, d, std=0.05 * scale / math.sqrt(d)) if q == 0 else randn(K, d, std=scale * 0.4 ** q / math.sqrt(d))
            pre = "%s.rvqs.0.layers.%d._codebook." % (st, q)
            sd[pre + "embed"] = e.float()[None]
            sd[pre + "initted"] = torch.tensor([True])
            sd[pre + "cluster_size"] = torch.ones(1, K)
            sd[pre + "embed_avg"] = e.float()[None].clone()
    return sd
