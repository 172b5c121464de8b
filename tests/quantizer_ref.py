"""float64 numpy restatement of upstream's learned quantizer in eval (sylber/model/quantizer.py: FFEncoder, _unit_norm /
_unit_norm_sep, Quantizer.forward / decode) with the GroupedResidualVQ look-up restated for one group of Euclidean codebooks.
The tests' oracle; contains no reference code.  ``sd`` is a ``Quantizer.state_dict()``-style dict (tensors or arrays), ``cfg`` the
constructor's keyword arguments."""
import numpy as np


def _a(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)


def geometry(cfg):
    enc = cfg["encoder_configs"]
    p = int(cfg.get("pitch_emb_dim", 8))
    return {"input_dim": int(enc["input_dim"]), "hidden_dims": [int(h) for h in enc["hidden_dims"]], "output_dim": int(enc["output_dim"]),
            "p": p, "A": int(enc["output_dim"]) - p, "Qa": int(cfg["art_vq_configs"]["num_quantizers"]),
            "Qp": int(cfg["pitch_vq_configs"]["num_quantizers"])}


def unit_norm(x):
    """_unit_norm: x / sqrt(sum x^2 + 1e-5)"""
    return x / np.sqrt((x ** 2).sum(-1, keepdims=True) + 1e-5)


def unit_norm_sep(x, separate, p):
    return np.concatenate([unit_norm(x[..., :-p]), unit_norm(x[..., -p:])], -1) if separate else unit_norm(x)


def encoder(x, sd, hidden_dims):
    """FFEncoder: per hidden dim Linear -> Linear -> ReLU -> Linear, then the output Linear"""
    def lin(x, name):
        return x @ _a(sd[name + ".weight"]).T + _a(sd[name + ".bias"])
    H = len(hidden_dims)
    for i in range(H):
        x = lin(x, "encoder.mlp.%d" % (2 * i))
        x = np.maximum(lin(x, "encoder.mlp.%d.0" % (2 * i + 1)), 0.0)
        x = lin(x, "encoder.mlp.%d.3" % (2 * i + 1))
    return lin(x, "encoder.mlp.%d" % (2 * H))


def codebooks(sd, stack, Q):
    out = []
    for q in range(Q):
        e = _a(sd["%s.rvqs.0.layers.%d._codebook.embed" % (stack, q)])
        out.append(e[0] if e.ndim == 3 else e)
    return out


def rvq_assign(x, books):
    """-> (ids [n, Q], z [n, d], gaps [n, Q]): per stage the nearest row (ties to the smallest index), z += E[i], r -= E[i].
    gaps[r, q]: (second-best - best squared distance) / (||r||^2 + max_k ||E_q[k]||^2), the relative margin of stage q's choice."""
    r = np.array(x, np.float64)
    z = np.zeros_like(r)
    n = len(r)
    ids = np.zeros((n, len(books)), np.int64)
    gaps = np.zeros((n, len(books)))
    for q, E in enumerate(books):
        d = (r ** 2).sum(1)[:, None] - 2 * r @ E.T + (E ** 2).sum(1)[None, :]
        i = np.argmin(d, 1)
        ids[:, q] = i
        if E.shape[0] > 1:
            part = np.partition(d, 1, axis=1)
            gaps[:, q] = (part[:, 1] - part[:, 0]) / ((r ** 2).sum(1) + (E ** 2).sum(1).max())
        else:
            gaps[:, q] = np.inf
        z = z + E[i]
        r = r - E[i]
    return ids, z, gaps


def forward(x, sd, cfg):
    """Quantizer.forward: {"indices", "quantize", "non_quantized", "gaps"} for x [n, input_dim]"""
    g = geometry(cfg)
    x = np.asarray(x, np.float64)
    blank = ~((x ** 2).sum(-1) > 0)
    t = unit_norm(x) if cfg.get("unit_norm_encoder_input", True) else x
    t = encoder(t, sd, g["hidden_dims"])
    sep = cfg.get("separate_norm", True)
    if cfg.get("unit_norm_encoder_output", True):
        t = unit_norm_sep(t, sep, g["p"])
    if cfg.get("keep_blank_zero", True):
        t[blank] = 0.0
    A = g["A"]
    ia, za, ga = rvq_assign(t[:, :A], codebooks(sd, "art_vq", g["Qa"]))
    ip, zp, gp = rvq_assign(t[:, A:], codebooks(sd, "pitch_vq", g["Qp"]))
    z = np.concatenate([za, zp], -1)
    if cfg.get("unit_norm_encoder_output", True):
        z = unit_norm_sep(z, sep, g["p"])
    return {"indices": np.concatenate([ia, ip], -1), "quantize": z, "non_quantized": t, "gaps": np.concatenate([ga, gp], -1)}


def decode(indices, sd, cfg):
    """Quantizer.decode: ids clipped at 0, each stack's rows summed in stage order, normalised as the encoder output"""
    g = geometry(cfg)
    ind = np.maximum(np.asarray(indices, np.int64), 0)
    parts = []
    for stack, lo, Q in (("art_vq", 0, g["Qa"]), ("pitch_vq", g["Qa"], g["Qp"])):
        books = codebooks(sd, stack, Q)
        z = 0.0
        for q, E in enumerate(books):
            z = z + E[ind[..., lo + q]]
        parts.append(z)
    z = np.concatenate(parts, -1)
    if cfg.get("unit_norm_encoder_output", True):
        z = unit_norm_sep(z, cfg.get("separate_norm", True), g["p"])
    return z
