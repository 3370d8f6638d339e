"""Worst error, in float32 ulp, of the device math library's powf / logf / expf as torch calls them, against float64, over the input
ranges the loss tests feed (tests/loss_ref.py takes POW_ULP and LOG_ULP from this: the figure rounded up to an integer, plus 1).
Measures the library, never the kernels under test.

    python tools/measure_pow_log_ulp.py
"""
import numpy as np
import torch

DEV = "cuda"
IG = float(np.float32(1.0 / float(np.float32(2.2))))                 # evd_crf_create's inv_gamma
IG1 = float(np.float32(np.float32(IG) - np.float32(1.0)))            # inv_gamma - 1.f


def ulp_err(got, ref):
    e = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126)))
    return (got.double() - ref).abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64, device=DEV), e - 23)


def sweep(name, fn, lo, hi):
    worst, arg = 0.0, None
    g = torch.Generator(device=DEV).manual_seed(1)
    for kind in ("log", "lin"):
        for _ in range(16):
            t = torch.rand(2 ** 20, generator=g, device=DEV, dtype=torch.float64)
            x = (torch.exp(np.log(lo) + t * (np.log(hi) - np.log(lo))) if kind == "log" else lo + t * (hi - lo)).float()
            err = ulp_err(fn(x), fn(x.double()))
            if float(err.max()) > worst:
                worst, arg = float(err.max()), float(x[err.argmax()])
    print(f"{name} on [{lo}, {hi}]: worst {worst:.4f} ulp at x = {arg!r}", flush=True)


if __name__ == "__main__":
    sweep("pow(x, 1/2.2)", lambda x: torch.pow(x, IG), 1e-4, 4.0)
    sweep("pow(x, 1/2.2 - 1)", lambda x: torch.pow(x, IG1), 1e-4, 4.0)
    sweep("log(x)", torch.log, 1e-5, 4.0)
    sweep("exp(-x)", lambda x: torch.exp(-x), 1e-3, 80.0)
