"""CPU model of conv layer 0's two 16-bit kernels against tests/frontend_ref.conv0_bound (no GPU needed).

Restates in numpy what conv0_mfma_kernel and conv0_gn_gelu_kernel<false, false> (csrc/frontend.hip) compute: the GroupNorm scale
folded into the taps in fp32, the waveform window and the taps as IEEE-half hi / lo pairs with exact products (matrix pipe) or fp32
operands (VALU), an fp32 accumulator that starts at the shift, gelu_fast, the bf16 / fp16 store.  The accumulation itself is done
in float64 and rounded once, so the model's error is a LOWER estimate of a kernel's; it shows which input scales stress the hi / lo
representation, not what the hardware returns (tests/test_gpu_frontend.py measures that).

    python tools/conv0_bound_model.py        prints max error / bound per input scale, format and kernel at 257 frames"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frontend_ref as fr                                   # noqa: E402
from sylber_amd.weights import synthetic_state_dict        # noqa: E402

f32 = np.float32


def gelu_fast(x):
    xc = np.clip(x, f32(-4.2), f32(4.2))
    u = xc * xc
    q = f32(6.949803233e-11) * u + f32(-6.356798643e-09)
    for c in (2.570604920e-07, -6.139445304e-06, 9.818511899e-05, -1.133762766e-03, 9.886963293e-03, -6.643489748e-02, 3.989362717e-01):
        q = q * u + f32(c)
    return x * (xc * q + f32(0.5))


def half(x):
    return x.astype(np.float16).astype(f32)


def main():
    w0, gw, gb = fr.conv0_weights(synthetic_state_dict(0, num_layers=1))
    base = fr.noise(1, 5 * 256 + 10, 11)
    cases = {"unit": base, "dc50": base + f32(50), "amp1e-3": base * f32(1e-3), "amp1e-5": base * f32(1e-5), "zeros": base * 0,
             "const": np.full_like(base, 0.5)}
    dot = lambda x, w: np.einsum("blj,bcj->blc", x.astype(np.float64), w.astype(np.float64))
    for name, wav in cases.items():
        ref = fr.conv0_ref(wav, w0, gw, gb)
        a32, b32 = ref["scale"].astype(f32), ref["shift"].astype(f32)
        X = fr.conv0_windows(wav).astype(f32)
        wp = (w0[None] * a32[:, :, None]).astype(f32)
        wh, xh = half(wp), half(X)
        wl, xl = half(wp - wh), half(X - xh)
        z_mfma = (b32[:, None].astype(np.float64) + dot(xh, wh) + dot(xl, wh) + dot(xh, wl)).astype(f32)
        z_valu = (b32[:, None].astype(np.float64) + dot(X, wp)).astype(f32)
        for fmt in ("bf16", "fp16"):
            r = [fr.worst_ratio(fr.round_fmt(gelu_fast(z).astype(np.float64), fmt), ref["y"], fr.conv0_bound(ref, fmt, k))[0]
                 for z, k in ((z_mfma, "mfma"), (z_valu, "valu"))]
            print("%-8s %s  matrix pipe %.3f  VALU %.3f" % (name, fmt, r[0], r[1]))


if __name__ == "__main__":
    main()
