"""Numpy restatements of ONE Adam step as include/hgs_rast.h defines it for hgs_adam_step (torch.optim.Adam without
weight decay, amsgrad or maximize).  The scalars are derived in double from (lr, beta1, beta2, eps, t) exactly as
humangaussian_amd/optim.py derives them; t is the step count AFTER its increment.

  step_fp32   every operation rounded to fp32, in the header's order: what the kernel must reproduce (the moments bit
              for bit - adds and multiplies only; the parameter up to the division's and the square root's last place)
  step_fp64   the same formulas in double on the fp32 inputs: the yardstick two fp32 implementations are measured by
"""
import math

import numpy as np


def scalars(lr, beta1, beta2, eps, t):
    """(step_size, bc2_sqrt, w1, beta2, w2, eps) in double."""
    return (lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), 1.0 - beta1, beta2, 1.0 - beta2, eps)


def step_fp32(p, g, m, v, lr, beta1, beta2, eps, t):
    """-> (p, m, v, u) float32 arrays after the step; u = step_size * (m / d), the update that was subtracted."""
    step_size, bc2_sqrt, w1, b2, w2, e = (np.float32(x) for x in scalars(lr, beta1, beta2, eps, t))
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m = m + (g - m) * w1
        v = v * b2 + (g * g) * w2
        d = np.sqrt(v) / bc2_sqrt + e
        u = step_size * (m / d)
        p = p - u
    assert all(x.dtype == np.float32 for x in (p, m, v, u))
    return p, m, v, u


def step_fp64(p, g, m, v, lr, beta1, beta2, eps, t):
    """-> (p, m, v) float64 arrays after the step (inputs of any float type, promoted to double)."""
    step_size, bc2_sqrt, w1, b2, w2, e = scalars(lr, beta1, beta2, eps, t)
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    m = m + (g - m) * w1
    v = v * b2 + (g * g) * w2
    d = np.sqrt(v) / bc2_sqrt + e
    return p - step_size * (m / d), m, v


def ulp(x):
    """spacing of fp32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, np.float32)))


def p_bound(u, p):
    """How far two fp32 evaluations of `p - u` may differ when their u differ only in the last places of one square root
    and two divisions (three roundings of 2^-24 relative each, on either side: <= 2^-21 |u| with room), plus the one
    rounding of the sum: 2^-21 |u| + ulp(p)."""
    return np.float64(2.0 ** -21) * np.abs(np.asarray(u, np.float64)) + ulp(p).astype(np.float64)


# the reference's six groups (gaussian_model.py:156-163 with the learning rates of its training arguments) and
# their trailing shapes at SH degree `deg`
REFERENCE_LRS = {"xyz": 1.6e-4, "f_dc": 0.0025, "f_rest": 0.0025 / 20.0, "opacity": 0.05, "scaling": 0.005,
                 "rotation": 0.001}


def reference_shapes(P, deg):
    return {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, (deg + 1) ** 2 - 1, 3), "opacity": (P, 1),
            "scaling": (P, 3), "rotation": (P, 4)}
