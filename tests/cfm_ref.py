"""Test-only functional restatement of the resynthesis decoder in torch: the flow-matching ``Regressor`` evaluated as
``ConditionalFlowMatcherWrapperRegressor.sample`` does (sylber/model/flowmatching.py:344-472, 581-688, 747-824) and the
fixed-grid midpoint sampler of ``torchdiffeq.odeint(method='midpoint')``.  ``sd`` uses the keys of ``Regressor.state_dict()``.

Eval-mode semantics only: ``cond = zeros`` and ``cond_mask = ones``, so the third ``to_embed`` block is exactly zero;
``self_attn_mask`` is None, so padded frames are ordinary frames.  Never imported by ``sylber_amd``.

Precision: everything runs in the dtype of ``sd`` and the inputs (fp32, or float64 with ``to_f64``).  Two things stay float32
because upstream defines them there and the decoder reproduces them bit for bit: the sampler's time grid
``torch.linspace(0, 1, steps)`` and the rotary angles ``pos * inv_freq`` (``RotaryEmbedding`` runs on its fp32 buffer, autocast
off); only their use is promoted.  The angles matter: the registers sit at position -10000, where one fp32 ulp of the angle is
5e-4 rad, and at the checkpoint's logit scale that moves a score by ~1 -- exact float64 angles put even torch's own fp32 forward
4e-3 .. 3e-2 (relative RMS) away at q / k gamma 1 .. 1.5.

``round16="bf16" | "fp16"`` (diagnosis only) rounds to that format exactly where the decoder's 16-bit kernels round
(csrc/cfm.hip): the cond operand and the to_embed cond block, the AdaRMSNorm outputs, the q / k / V operands of attention (q after
its ``10 * log2(e)`` pre-scaling), the attention context, the GEGLU output and the weights of every GEMM (qkv, out, FF1, FF2).
What stays unrounded is what the kernels keep in fp32: the y path of to_embed, the conv, the residual stream, the time
conditioning, the final norm and to_pred.  (The kernels' probabilities are rounded too, inside the attention; that rounding
depends on the kernel's running maximum and is not restated.)"""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634


def to_f64(sd):
    """a float64 copy of a state dict (integer tensors unchanged)"""
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _rounder(round16):
    if round16 is None:
        return lambda u: u
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[round16]
    return lambda u: u.to(dt).to(u.dtype)


def time_conditioning(sd, t):
    """t: float -> the 2048-wide ``sinu_pos_emb`` output for one time (the same for every row)"""
    w = sd["sinu_pos_emb.0.weights"]
    x = torch.tensor([float(t)], dtype=w.dtype, device=w.device)
    freqs = x[:, None] * w[None, :] * 2 * math.pi
    emb = torch.cat((freqs.sin(), freqs.cos()), dim=-1)
    return F.silu(F.linear(emb, sd["sinu_pos_emb.1.weight"], sd["sinu_pos_emb.1.bias"]))     # [1, 2048]


def _ada_rmsnorm(x, sd, p, temb):
    gamma = F.linear(temb, sd[p + ".to_gamma.weight"], sd[p + ".to_gamma.bias"])[:, None]
    beta = F.linear(temb, sd[p + ".to_beta.weight"], sd[p + ".to_beta.bias"])[:, None]
    return F.normalize(x, dim=-1) * (x.shape[-1] ** 0.5) * gamma + beta


def _rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def evaluate(sd, y, t, cond_emb, heads=8, registers=16, round16=None):
    """one velocity evaluation: y [B,T,14], t float, cond_emb [B,T,256] -> v [B,T,14]"""
    r16 = _rounder(round16)
    B, T, _ = y.shape
    pin_w, pin_b = sd["proj_in.weight"], sd["proj_in.bias"]
    zero = F.linear(torch.zeros_like(y), pin_w, pin_b) * 0.0
    if round16 is None:
        x = F.linear(torch.cat([F.linear(y, pin_w, pin_b), cond_emb, zero], dim=-1), sd["to_embed.weight"], sd["to_embed.bias"])
    else:
        ew, P = sd["to_embed.weight"], pin_w.shape[0]
        x = (F.linear(F.linear(y, pin_w, pin_b), ew[:, :P]) + F.linear(r16(cond_emb), r16(ew[:, P:P + cond_emb.shape[-1]]))
             + sd["to_embed.bias"])
    cw, cb = sd["conv_embed.dw_conv1d.0.weight"], sd["conv_embed.dw_conv1d.0.bias"]
    conv = F.gelu(F.conv1d(x.transpose(1, 2), cw, cb, padding=cw.shape[-1] // 2, groups=cw.shape[0])).transpose(1, 2)
    x = conv + x
    temb = time_conditioning(sd, t).expand(B, -1)
    x = torch.cat([sd["transformer.register_tokens"][None].expand(B, -1, -1), x], dim=1)
    inv_freq = sd["transformer.rotary_emb.inv_freq"]
    pos = torch.cat([torch.full((registers,), -10000, dtype=torch.long), torch.arange(T)]).to(inv_freq.device, torch.float32)
    freqs = torch.einsum("i , j -> i j", pos, inv_freq.float()).to(inv_freq.dtype)     # angles in fp32 as upstream's buffer
    freqs = torch.cat((freqs, freqs), dim=-1)
    depth = len({k.split(".")[2] for k in sd if k.startswith("transformer.layers.")})
    for i in range(depth):
        p = "transformer.layers.%d." % i
        h = r16(_ada_rmsnorm(x, sd, p + "2", temb))
        q, k, v = F.linear(h, r16(sd[p + "3.to_qkv.weight"])).chunk(3, dim=-1)
        q, k, v = (u.reshape(B, -1, heads, u.shape[-1] // heads).transpose(1, 2) for u in (q, k, v))
        dh = q.shape[-1]
        q = F.normalize(q, dim=-1) * sd[p + "3.q_norm.gamma"] * (dh ** 0.5)
        k = F.normalize(k, dim=-1) * sd[p + "3.k_norm.gamma"] * (dh ** 0.5)
        q = q * freqs.cos() + _rotate_half(q) * freqs.sin()
        k = k * freqs.cos() + _rotate_half(k) * freqs.sin()
        if round16 is None:
            sim = torch.einsum("b h i d, b h j d -> b h i j", q, k) * 10
        else:       # the kernels' operands: q pre-scaled into log2 units, then rounded; k and V rounded
            sim = torch.einsum("b h i d, b h j d -> b h i j", r16(q * (10 * LOG2E)), r16(k)) / LOG2E
            v = r16(v)
        o = torch.einsum("b h i j, b h j d -> b h i d", sim.softmax(dim=-1), v)
        o = o.transpose(1, 2).reshape(B, -1, heads * dh)
        x = F.linear(r16(o), r16(sd[p + "3.to_out.weight"])) + x
        h = r16(_ada_rmsnorm(x, sd, p + "4", temb))
        a, gate = F.linear(h, r16(sd[p + "5.0.weight"]), sd[p + "5.0.bias"]).chunk(2, dim=-1)
        x = F.linear(r16(F.gelu(gate) * a), r16(sd[p + "5.3.weight"]), sd[p + "5.3.bias"]) + x
    x = x[:, registers:]
    x = F.normalize(x, dim=-1) * (x.shape[-1] ** 0.5) * sd["transformer.final_norm.gamma"]
    return F.linear(x, sd["to_pred.weight"])


def sample(sd, cond_emb, steps=5, y0=None, pitch_amp=None, round16=None):
    """``cfm_wrapper.sample`` with ``torchdiffeq``'s fixed-grid midpoint rule on ``t = linspace(0, 1, steps)``:
    per interval ``y_mid = y + f(t0, y) * (dt / 2)``, ``y += dt * f(t0 + dt / 2, y_mid)``.  ``steps == 1`` returns ``y0``.
    ``pitch_amp``: divide channel 12 by it afterwards (``resynthesize``)."""
    B, T, _ = cond_emb.shape
    y = torch.zeros(B, T, 14, dtype=cond_emb.dtype, device=cond_emb.device) if y0 is None else y0.clone()
    if steps > 1:
        t = torch.linspace(0, 1, steps)                  # float32 as upstream; y (float64) * a float32 0-dim tensor stays float64
        for i in range(steps - 1):
            t0, dt = t[i], t[i + 1] - t[i]
            half = 0.5 * dt
            ymid = y + evaluate(sd, y, float(t0), cond_emb, round16=round16) * half
            y = y + dt * evaluate(sd, ymid, float(t0 + half), cond_emb, round16=round16)
    if pitch_amp is not None:
        y = y.clone()
        y[..., 12] = y[..., 12] / pitch_amp
    return y
