"""Restatements for the conditional LayerNorm and the device noise (csrc/cond_layer_norm.hip), sharing no code with the package.

* :func:`cond_layer_norm` -- the layer in f64 torch; gradients come from torch autograd on it.
* :func:`philox4x32_10`, :func:`noise_words`, :func:`gaussian_noise` -- the generator of ``anemoi_gaussian_noise`` in numpy: the
  integers exactly (Philox4x32-10, Salmon et al. 2011), the Box-Muller normals in f64.
* :func:`moment_report` / :func:`moment_bounds` -- the moments the tests bound, and the 6 sigma bounds of iid normals.
"""

import math

import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
NOISE_KEY1 = 0x6E6F6973
MASK = np.uint64(0xFFFFFFFF)
MAX_ABS = math.sqrt(2.0 * 24.0 * math.log(2.0))  # u1 >= 2^-24


def cond_layer_norm(x, cond, w_scale, b_scale, w_bias, b_bias, eps=1e-5):
    """``xhat * (1 + cond w_scale^T + b_scale) + (cond w_bias^T + b_bias)``, biased variance, everything in f64."""
    x, cond, w_scale, b_scale, w_bias, b_bias = (t.double() for t in (x, cond, w_scale, b_scale, w_bias, b_bias))
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    xh = (x - mean) / torch.sqrt(var + eps)
    return xh * (1.0 + cond @ w_scale.T + b_scale) + (cond @ w_bias.T + b_bias)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays holding 32-bit words; the key is bumped after every round."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def noise_words(n, seed, word=0):
    """The 32-bit word pairs ``(wa, wb)`` ``[n]`` of the elements ``0 .. n - 1``: quad ``q = i // 4`` has the counter ``(q, q >>
    32, 0, 0)`` and the key ``(seed + word mod 2^32, NOISE_KEY1)``; its words ``w0 w1`` serve the elements ``4 q, 4 q + 1``, ``w2
    w3`` the next two."""
    quads = (n + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    zero = np.zeros(quads, dtype=np.uint64)
    w = philox4x32_10(q & MASK, q >> np.uint64(32), zero, zero, (int(seed) + int(word)) & 0xFFFFFFFF, NOISE_KEY1)
    wa = np.stack([w[0], w[0], w[2], w[2]], axis=1).reshape(-1)[:n]
    wb = np.stack([w[1], w[1], w[3], w[3]], axis=1).reshape(-1)[:n]
    return wa, wb


def gaussian_noise(rows, k, std=1.0, *, seed, word=0):
    """f64 ``[rows, k]``: ``u1 = ((wa >> 8) + 1) / 2^24``, ``u2 = (wb >> 8) / 2^24``, even elements ``sqrt(-2 ln u1) cos(2 pi u2)``,
    odd elements the sine."""
    n = rows * k
    wa, wb = noise_words(n, seed, word)
    u1 = ((wa >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0**24
    u2 = (wb >> np.uint64(8)).astype(np.float64) / 2.0**24
    r = np.sqrt(-2.0 * np.log(u1))
    odd = (np.arange(n) & 1).astype(bool)
    z = r * np.where(odd, np.sin(2.0 * np.pi * u2), np.cos(2.0 * np.pi * u2))
    return (float(std) * z).reshape(rows, k)


def _lag1(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt(float((a * a).mean()) * float((b * b).mean())))


def moment_report(z):
    """mean, var - 1, m4 - 3, lag-1 correlation along a row and down a column, largest magnitude of ``z [rows, k]`` (f64)."""
    z = np.asarray(z, dtype=np.float64)
    mean = float(z.mean())
    d = z - mean
    var = float((d * d).mean())
    m4 = float((d**4).mean())  # the raw fourth central moment: its variance is (105 - 9) / n
    return {"mean": mean, "var": var - 1.0, "m4": m4 - 3.0, "lag_row": _lag1(z[:, :-1], z[:, 1:]),
            "lag_col": _lag1(z[:-1, :], z[1:, :]), "max": float(np.abs(z).max())}


def moment_bounds(n):
    """6 sigma of n iid standard normals: sd(mean) = 1 / sqrt n, sd(var) = sqrt(2 / n), sd(m4) = sqrt(96 / n), sd(corr) = 1 / sqrt n;
    no value beyond sqrt(2 * 24 * ln 2)."""
    return {"mean": 6.0 / math.sqrt(n), "var": 6.0 * math.sqrt(2.0 / n), "m4": 6.0 * math.sqrt(96.0 / n),
            "lag_row": 6.0 / math.sqrt(n), "lag_col": 6.0 / math.sqrt(n), "max": MAX_ABS}


def check_moments(z, what=""):
    rep, bounds = moment_report(z), moment_bounds(z.size)
    print(f"noise moments {what}: " + ", ".join(f"{k} {v:+.3e} (bound {bounds[k]:.3e})" for k, v in rep.items()))
    for k, v in rep.items():
        assert abs(v) < bounds[k] or (k == "max" and abs(v) <= bounds[k]), (what, k, v, bounds[k])


NOISE_SEEDS = (1, 20240229, 0x7FFFFFFE)
