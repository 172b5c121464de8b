"""Golden vectors for the resynthesis decoder (CPU only; survey container only, never on the GPU box): runs the REFERENCE's
own ``Regressor`` and ``ConditionalFlowMatcherWrapperRegressor.sample`` (sylber/model/flowmatching.py:474-824) at the
sylber_resynthesis.yaml geometry, built with ``synthetic_regressor_state_dict(0)`` loaded ``strict=True``, and writes
tests/golden/cfm_decoder.npz (weights are NOT stored: tests regenerate them from the seed).

What is stubbed (not installed here, and not on the inference path): ``torchode``, ``beartype``, ``gateloop_transformer``, and
``torchdiffeq`` -- whose ``odeint`` is replaced by ``_odeint_midpoint`` below, the documented fixed-grid midpoint rule
torchdiffeq applies for ``method='midpoint'`` on a given time grid.  Contains no reference code.

Cases:
  * ``eval_t{0,1}``: one velocity evaluation (``forward_with_cond_scale``) at two times on a 2 x 40 batch;
  * ``s{1,2,5}_zero`` / ``s{1,2,5}_y0``: ``sample`` at steps 1, 2, 5 with ``rand_scale = 0`` and with a stored ``y0``
    (``torch.randn_like`` patched to return it);
  * ``ragged``: 3 clips of 100 / 230 / 300 frames, zero-padded to 300, ``sample(steps=5)`` on the padded batch;
  * ``feat``: the ``features=`` branch of ``SegmentSynthesis.resynthesize`` (MLP conditioner of
    ``synthetic_mlp_state_dict(1)``, silence mask, decoder, pitch scaling by ``pitch_amp = 5``);
  * ``thr``: ``Thresholder.get_threshold()`` at the yaml's statistics."""
import importlib
import json
import os
import sys
import typing

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict  # noqa: E402
from tools import ref_shim                                                             # noqa: E402
from tools.gen_golden_mlp import _stub                                                 # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cfm_decoder.npz")
YAML_REGRESSOR = dict(depth=8, sigma=0.0, dim_head=64, heads=8, dim=512, dim_in_proj=64, dim_cond_emb=256)
YAML_THRESHOLDER = dict(signal_mean=6.10, signal_var=0.87, noise_mean=0.3879, noise_var=0.6819)


def _odeint_midpoint(func, y0, t, **_):
    """torchdiffeq.odeint(func, y0, t, method='midpoint') on the fixed grid t: per interval
    f0 = func(t0, y); y_mid = y + f0 * (dt / 2); y1 = y + dt * func(t0 + dt / 2, y_mid).  Returns the trajectory."""
    out = [y0]
    y = y0
    for i in range(len(t) - 1):
        t0, t1 = t[i], t[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        f0 = func(t0, y)
        y_mid = y + f0 * half_dt
        y = y + dt * func(t0 + half_dt, y_mid)
        out.append(y)
    return torch.stack(out)


def load_reference():
    ref_shim.load()
    _stub("torchode", Tsit5=object)
    _stub("torchdiffeq", odeint=_odeint_midpoint)
    bt = _stub("beartype", beartype=lambda f: f)
    bt.typing = _stub("beartype.typing", Tuple=typing.Tuple, Union=typing.Union, Optional=typing.Optional, List=typing.List)
    _stub("gateloop_transformer", SimpleGateLoopLayer=object)
    _stub("vector_quantize_pytorch", GroupedResidualVQ=object)
    _stub("lightning", LightningModule=torch.nn.Module)
    fm = importlib.import_module("sylber.model.flowmatching")
    fm.odeint = _odeint_midpoint
    return fm


def build_wrapper(fm, seed=0):
    reg = fm.Regressor(**YAML_REGRESSOR).eval()
    reg.load_state_dict(synthetic_regressor_state_dict(seed), strict=True)
    return fm.ConditionalFlowMatcherWrapperRegressor(regressor=reg, sigma=0.0).eval()


def golden_inputs():
    """the seeded conditioning inputs / noise of every case (tests regenerate nothing from these: they are stored)"""
    g = torch.Generator().manual_seed(7)
    cond = torch.randn(2, 40, 256, generator=g)
    cond[1, 30:] = 0.0                                      # silence-masked frames, as the conditioner leaves them
    x = torch.randn(2, 40, 14, generator=g)
    y0 = torch.randn(2, 40, 14, generator=g) * 0.7
    lens = [100, 230, 300]
    rag = torch.zeros(3, 300, 256)
    for b, n in enumerate(lens):
        rag[b, :n] = torch.randn(n, 256, generator=g)
    feat = torch.randn(2, 37, 768, generator=g)
    feat[0, 3] = 0.0
    feat[1, 10] = 5e-6
    return dict(cond=cond, x=x, y0=y0, rag_cond=rag, rag_lens=np.asarray(lens, np.int32), feat=feat)


def sample_with(wrapper, cond, steps, y0=None):
    orig = torch.randn_like
    if y0 is not None:
        torch.randn_like = lambda t, *a, **k: y0.clone()
    try:
        return wrapper.sample(cond_emb=cond, steps=steps, rand_scale=1.0 if y0 is not None else 0.0)
    finally:
        torch.randn_like = orig


def main():
    fm = load_reference()
    seg_mod = importlib.import_module("sylber.model.segment_synthesis")
    su = importlib.import_module("sylber.utils.segment_utils")
    w = build_wrapper(fm)
    inp = golden_inputs()
    out = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in inp.items()}
    meta = {"weights": "synthetic_regressor_state_dict(0)", "regressor_configs": YAML_REGRESSOR, "cases": {}}
    with torch.inference_mode():
        for i, t in enumerate((0.25, 0.625)):
            v = w.regressor.forward_with_cond_scale(inp["x"], times=torch.tensor(t), cond_token_ids=None,
                                                    cond=torch.zeros(2, 40, 14), cond_emb=inp["cond"])
            out["eval_t%d" % i] = v.numpy()
            out["eval_t%d_time" % i] = np.float32(t)
        for steps in (1, 2, 5):
            out["s%d_zero" % steps] = sample_with(w, inp["cond"], steps).numpy()
            out["s%d_y0" % steps] = sample_with(w, inp["cond"], steps, inp["y0"]).numpy()
        out["ragged"] = sample_with(w, inp["rag_cond"], 5).numpy()

        # the features= branch of SegmentSynthesis.resynthesize, run on an object whose members are the real MLP and wrapper
        syn = object.__new__(seg_mod.SegmentSynthesis)
        torch.nn.Module.__init__(syn)
        mlp = seg_mod.MLP(768, output_dim=256, hidden_dims=[512, 512]).eval()
        mlp.load_state_dict(synthetic_mlp_state_dict(1), strict=True)
        syn.input_model = mlp
        syn.cfm_wrapper = w
        syn.pitch_amp = 5
        syn.quantizer = None
        art, segs = syn.resynthesize(features=inp["feat"], steps=5, rand_scale=0.0)
        assert segs is None
        out["feat_art"] = art.numpy()

        thr = su.Thresholder(**YAML_THRESHOLDER)
        out["thr"] = np.float32(thr.get_threshold().item())
    meta["cases"] = sorted(k for k in out if k not in inp)
    meta["thr_stats"] = YAML_THRESHOLDER
    out["meta_json"] = np.asarray(json.dumps(meta, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
