"""Plain numpy fp64 reference for ``K.fm_step`` (K25) and the fp32 yardstick the device tests measure it against.

The model is Spark's factorization machine: factors V [d][k], linear weights w [d], intercept b, in Spark's flat
vector (V row-major, then w if fitLinear, then b if fitIntercept).  The reference forms the raw prediction in the
*pairwise* form b + w.x + sum_{i<j} <v_i, v_j> x_i x_j and differentiates that; the kernel and the host formulation
use the sum-of-squares form.  Written independently of the package code.
"""
import functools

import numpy as np
import torch

SQUARED, LOGISTIC = 0, 1


def num_params(d, k, lin=True, icpt=True):
    return d * k + (d if lin else 0) + (1 if icpt else 0)


def unpack(theta, d, k, lin=True, icpt=True):
    theta = np.asarray(theta, dtype=np.float64)
    V = theta[:d * k].reshape(d, k)
    w = theta[d * k:d * k + d] if lin else np.zeros(d)
    b = theta[d * k + (d if lin else 0)] if icpt else 0.0
    return V, w, float(b)


def raw(X, theta, k, lin=True, icpt=True):
    """b + w.x + sum_{i<j} <v_i, v_j> x_i x_j: the strict upper triangle of the Gram matrix of the factors."""
    X = np.asarray(X, dtype=np.float64)
    V, w, b = unpack(theta, X.shape[1], k, lin, icpt)
    U = np.triu(V @ V.T, 1)
    return b + X @ w + np.einsum("ri,ij,rj->r", X, U, X)


def loss_and_multiplier(r, y, loss):
    if loss == SQUARED:
        return (r - y) ** 2, 2.0 * (r - y)
    z = np.where(y > 0, -r, r)
    with np.errstate(over="ignore"):
        sig = np.where(r >= 0, 1.0 / (1.0 + np.exp(-np.abs(r))), np.exp(-np.abs(r)) / (1.0 + np.exp(-np.abs(r))))
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))), sig - y


def step(X, y, theta, k, loss, lin=True, icpt=True, mask=None):
    """(loss sum, gradient sum [P], count) over the rows of ``mask`` (all), un-normalised.  The gradient of the
    pairwise form: d raw / d v_i = x_i sum_{j != i} v_j x_j."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if mask is not None:
        X, y = X[mask], y[mask]
    n, d = X.shape
    V, w, b = unpack(theta, d, k, lin, icpt)
    l, m = loss_and_multiplier(raw(X, theta, k, lin, icpt), y, loss)
    gV = np.zeros((d, k))
    for i in range(d):
        others = X @ V - np.outer(X[:, i], V[i])            # sum_{j != i} v_j x_j per row
        gV[i] = ((m * X[:, i])[:, None] * others).sum(0)
    parts = [gV.reshape(-1)] + ([X.T @ m] if lin else []) + ([np.array([m.sum()])] if icpt else [])
    return float(l.sum()), np.concatenate(parts), n


def yardstick(X, y, theta, k, loss, lin=True, icpt=True, mask=None):
    """The kernel's sum-of-squares formulation in plain torch fp32 on the CPU, parameters rounded to fp32.  Returns
    (loss sum, gradient sum [P], raw [n]) as fp64 numpy; the sums over the rows of ``mask``, raw for every row."""
    d = np.asarray(X).shape[1]
    V, w, b = (torch.tensor(np.asarray(t), dtype=torch.float32) for t in unpack(theta, d, k, lin, icpt))
    Xt = torch.tensor(np.asarray(X), dtype=torch.float32)
    yt = torch.tensor(np.asarray(y), dtype=torch.float32)
    S = Xt @ V
    r = b + Xt @ w + 0.5 * ((S * S).sum(1) - ((Xt * Xt) @ (V * V)).sum(1))
    if loss == SQUARED:
        l, m = (r - yt) ** 2, 2.0 * (r - yt)
    else:
        z = torch.where(yt > 0, -r, r)
        l, m = z.clamp_min(0) + torch.log1p(torch.exp(-z.abs())), torch.sigmoid(r) - yt
    if mask is not None:
        keep = torch.tensor(np.asarray(mask))
        l, m = torch.where(keep, l, torch.zeros_like(l)), torch.where(keep, m, torch.zeros_like(m))
    gV = Xt.T @ (S * m[:, None]) - V * ((Xt * Xt).T @ m)[:, None]
    parts = [gV.reshape(-1)] + ([Xt.T @ m] if lin else []) + ([m.sum().reshape(1)] if icpt else [])
    return float(l.double().sum()), torch.cat(parts).double().numpy(), r.double().numpy()


def make_case(d, k, n, loss, seed=0, lin=True, icpt=True, dtype=np.float32, scale=1.0):
    """(X, y, theta): Gaussian rows, factors of a size that makes the interaction term O(1), labels real (squared) or
    0 / 1 (logistic); theta rounded to fp32 so that the device op (defined at the fp32-rounded parameters) and the
    reference share it exactly."""
    rng = np.random.default_rng(seed + 1000 * d + 10 * k + n)
    X = rng.normal(size=(n, d)).astype(dtype)
    theta = np.zeros(num_params(d, k, lin, icpt))
    theta[:d * k] = rng.normal(scale=scale * 0.7 / (d * k) ** 0.25, size=d * k)
    if lin:
        theta[d * k:d * k + d] = rng.normal(scale=scale / np.sqrt(d), size=d)
    if icpt:
        theta[-1] = 0.3 * scale
    y = rng.normal(size=n) if loss == SQUARED else rng.integers(0, 2, n).astype(np.float64)
    return X, y, theta.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(d, k, n, loss, seed=0, lin=True, icpt=True):
    """make_case with its reference and yardstick results, computed once and shared (treat as read-only)."""
    X, y, theta = make_case(d, k, n, loss, seed, lin, icpt)
    ls, g, _ = step(X, y, theta, k, loss, lin, icpt)
    yl, yg, yr = yardstick(X, y, theta, k, loss, lin, icpt)
    return dict(X=X, y=y, theta=theta, loss=ls, grad=g, raw=raw(X, theta, k, lin, icpt), y_loss=yl, y_grad=yg,
                y_raw=yr)


def product_data(n=600, d=4, seed=0):
    """Gaussian x, y = x1 x2 + x3, no noise: a linear model explains x3 and nothing of the product (std 1)."""
    X = np.random.default_rng(seed).normal(size=(n, d))
    return X, X[:, 0] * X[:, 1] + X[:, 2]


def sign_data(n=600, d=3, seed=0):
    """Gaussian x, label = [x1 x2 > 0]: no linear boundary does better than chance."""
    X = np.random.default_rng(seed).normal(size=(n, d))
    return X, (X[:, 0] * X[:, 1] > 0).astype(np.float64)
