"""Golden vectors for the learned quantizer (CPU only; survey container only, never on the GPU box): runs the REFERENCE's own
``Quantizer.forward``, ``get_indices``, ``decode`` and ``load_quantizer`` (sylber/model/quantizer.py), loaded in the manner of
tools/ref_shim.py, and writes tests/golden/quantizer.npz.

``vector_quantize_pytorch`` is not installed, so it is stubbed by a module whose ``GroupedResidualVQ`` implements the restated eval
semantics for one group (r = x; per stage i = argmin_k ||r - E[k]||, z += E[i], r -= E[i]; the state-dict buffers of a trained
checkpoint).  Everything upstream owns is pinned by running its code: the layer order of FFEncoder, both epsilons, separate_norm,
the blank mask, the index layout and decode's clip and norm.  The look-up itself stays parity unpinned, as for KMQuantizer.

Two configs: (a) 768 -> [512] -> 72 (A = 64, p = 8), art 4 x 1024, pitch 2 x 64; (b) odd sizes 100 -> [200, 96] -> 45 (A = 37),
one stage of K = 3 per stack, separate_norm=False, unit_norm_encoder_input=False, small biases.  Weights come from
``synthetic_quantizer_state_dict(cfg, seed)`` (the fixture stores a checksum of them, not the tensors).  Rows: random tokens at
several scales, blank rows, tiny rows whose normalised input (a) or encoder output (b) is far from unit norm (the 1e-5 epsilon
matters); rows with a float64 best-to-second margin under 1e-4 at any stage are dropped, so the ids are exact.
Contains no reference code."""
import hashlib
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quantizer_ref as R                                                       # noqa: E402
from sylber_amd.weights import synthetic_quantizer_state_dict                   # noqa: E402
from tools import ref_shim                                                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "quantizer.npz")

CONFIGS = {
    "a": dict(seed=0, bias_std=0.01, cfg=dict(
        encoder_configs=dict(input_dim=768, hidden_dims=[512], output_dim=72, dropout=0.1),
        art_vq_configs=dict(dim=64, codebook_size=1024, num_quantizers=4, groups=1, decay=0.99, commitment_weight=1.0,
                            kmeans_init=True, threshold_ema_dead_code=2, quantize_dropout=False),
        pitch_vq_configs=dict(dim=8, codebook_size=64, num_quantizers=2, groups=1, decay=0.99),
        pitch_emb_dim=8)),
    "b": dict(seed=1, bias_std=2e-4, cfg=dict(
        encoder_configs=dict(input_dim=100, hidden_dims=[200, 96], output_dim=45),
        art_vq_configs=dict(dim=37, codebook_size=3, num_quantizers=1),
        pitch_vq_configs=dict(dim=8, codebook_size=3, num_quantizers=1),
        pitch_emb_dim=8, separate_norm=False, unit_norm_encoder_input=False)),
}


class _Codebook(torch.nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self.register_buffer("initted", torch.tensor([False]))
        self.register_buffer("cluster_size", torch.zeros(1, codebook_size))
        self.register_buffer("embed_avg", torch.zeros(1, codebook_size, dim))
        self.register_buffer("embed", torch.zeros(1, codebook_size, dim))


class _Layer(torch.nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self._codebook = _Codebook(dim, codebook_size)


class _RVQ(torch.nn.Module):
    def __init__(self, dim, codebook_size, num_quantizers):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Layer(dim, codebook_size) for _ in range(num_quantizers)])


class GroupedResidualVQ(torch.nn.Module):
    """the restated eval semantics of vector_quantize_pytorch's GroupedResidualVQ for groups = 1 (ids picked in float64: the
    fixture keeps only rows without near-ties, where any exact arithmetic agrees)"""

    def __init__(self, dim, codebook_size, num_quantizers, groups=1, **training_only):
        super().__init__()
        assert groups == 1
        self.rvqs = torch.nn.ModuleList([_RVQ(dim, codebook_size, num_quantizers)])

    def _books(self):
        return [layer._codebook.embed[0] for layer in self.rvqs[0].layers]

    def forward(self, x):
        r = x.clone()
        z = torch.zeros_like(x)
        ids = []
        for E in self._books():
            d = torch.cdist(r.double().reshape(-1, r.shape[-1]), E.double()).reshape(r.shape[:-1] + (E.shape[0],))
            i = d.argmin(-1)
            e = E[i]
            z = z + e
            r = r - e
            ids.append(i)
        return z, torch.stack(ids, -1)[None], torch.zeros(())

    def get_output_from_indices(self, indices):
        ind = indices[0]
        z = 0.0
        for q, E in enumerate(self._books()):
            z = z + E[ind[..., q]]
        return z


def load_reference():
    if not ref_shim.available():
        raise RuntimeError("reference checkout not present at %s" % ref_shim.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    if "sylber" not in sys.modules:
        pkg = types.ModuleType("sylber")
        pkg.__path__ = [os.path.join(ref_shim.REFERENCE_ROOT, "sylber")]
        sys.modules["sylber"] = pkg
    vq = types.ModuleType("vector_quantize_pytorch")
    vq.GroupedResidualVQ = GroupedResidualVQ
    sys.modules["vector_quantize_pytorch"] = vq
    return importlib.import_module("sylber.model.quantizer")


def state_dict_sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()


def tokens(case, D, rng):
    rows = [rng.standard_normal((40, D)) * rng.choice([0.3, 1.0, 4.0], (40, 1)),
            np.zeros((3, D)),                                              # blank rows
            rng.standard_normal((12, D)) * (1e-4 if case == "a" else 3e-5)]  # tiny rows: the 1e-5 epsilon matters
    x = np.concatenate(rows).astype(np.float32)
    x[-1, :] = 0.0
    x[-1, 5] = 1e-3                                                        # one nonzero column only
    return x


def main():
    qm = load_reference()
    out = {}
    meta = {}
    for case, spec in CONFIGS.items():
        cfg = spec["cfg"]
        sd = synthetic_quantizer_state_dict(cfg, spec["seed"], bias_std=spec["bias_std"])
        # the reference's own loader, from a {"config", "state_dict"} checkpoint (strict=True)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "q.ckpt")
            torch.save({"config": cfg, "state_dict": sd}, path)
            q = qm.load_quantizer(config=path)
        assert not q.training
        rng = np.random.default_rng(100 + spec["seed"])
        x = tokens(case, cfg["encoder_configs"]["input_dim"], rng)
        ref = R.forward(x, sd, cfg)
        keep = (ref["gaps"] > 1e-4).all(1)
        x = x[keep]
        with torch.no_grad():
            o = q(torch.from_numpy(x))
            ids = q.get_indices(torch.from_numpy(x))
            assert torch.equal(ids, o["indices"])
            bad = ids.clone()
            bad[::3, 0] = -1                                                    # decode clips negative ids to 0
            bad[1::3, -1] = -5
            dec = q.decode(bad)
        ref = R.forward(x, sd, cfg)
        assert np.array_equal(o["indices"].numpy(), ref["indices"])
        nq = o["non_quantized"].numpy()
        # the fixture covers what its docstring promises
        assert (np.abs(nq[(x ** 2).sum(1) == 0]) == 0).all() and ((x ** 2).sum(1) == 0).sum() == 3
        enc_norm = np.sqrt((ref["non_quantized"].astype(np.float64) ** 2).sum(1))
        meta[case] = {"seed": spec["seed"], "bias_std": spec["bias_std"], "cfg": cfg, "sd_sha256": state_dict_sha(sd),
                      "rows": int(len(x)), "dropped": int((~keep).sum()), "min_output_norm_nonblank": float(enc_norm[enc_norm > 0].min())}
        out.update({case + "_tokens": x, case + "_indices": o["indices"].numpy().astype(np.int64), case + "_non_quantized": nq,
                    case + "_quantize": o["quantize"].numpy(), case + "_decode_ids": bad.numpy().astype(np.int64),
                    case + "_decode": dec.numpy()})
        print(case, meta[case])
    out["meta_json"] = np.asarray(json.dumps(meta, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
