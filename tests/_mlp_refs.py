"""Plain numpy fp64 reference for ``K.mlp_step`` (K24) and the fp32 yardstick the device tests measure it against.

The net is Spark's MultilayerPerceptronClassifier: affine layers, sigmoid after every layer but the last, softmax
with cross-entropy on top; the weights are Spark's flat vector (per layer W [out, in] column-major, entry (o, i) at
off + o + i * out, then the out biases).  Written independently of the package code.
"""
import functools

import numpy as np
import torch


def num_params(layers):
    return sum(o * i + o for i, o in zip(layers[:-1], layers[1:]))


def unpack(theta, layers):
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        W = np.empty((o, i))
        for col in range(i):
            W[:, col] = theta[off + col * o: off + (col + 1) * o]
        out.append((W, theta[off + o * i: off + o * i + o].copy()))
        off += o * i + o
    return out


def pack(grads):
    return np.concatenate([np.concatenate([gW.reshape(-1, order="F"), gb]) for gW, gb in grads])


def forward(X, theta, layers):
    """(activations [a_0 .. a_{L-1}], logits), fp64."""
    acts = [np.asarray(X, dtype=np.float64)]
    Wb = unpack(np.asarray(theta, dtype=np.float64), layers)
    for l, (W, b) in enumerate(Wb):
        z = acts[-1] @ W.T + b
        if l == len(Wb) - 1:
            return acts, z
        with np.errstate(over="ignore"):
            acts.append(1.0 / (1.0 + np.exp(-z)))


def softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def step(X, y, theta, layers):
    """(loss sum, gradient sum [P]) over the rows, un-normalised."""
    theta = np.asarray(theta, dtype=np.float64)
    Wb = unpack(theta, layers)
    acts, z = forward(X, theta, layers)
    n = z.shape[0]
    y = np.asarray(y, dtype=np.int64)
    m = z.max(1) if n else np.zeros(0)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    loss = float((lse - z[np.arange(n), y]).sum())
    D = softmax(z) if n else z
    D[np.arange(n), y] -= 1.0
    grads = [None] * len(Wb)
    for l in range(len(Wb) - 1, -1, -1):
        grads[l] = (D.T @ acts[l], D.sum(0))
        if l > 0:
            D = (D @ Wb[l][0]) * acts[l] * (1.0 - acts[l])
    return loss, pack(grads)


def predict(X, theta, layers):
    """(raw, prob, pred): pred the lowest index among equals."""
    _, z = forward(X, theta, layers)
    return z, (softmax(z) if z.shape[0] else z), np.argmax(z, 1).astype(np.int32)


def yardstick(X, y, theta, layers):
    """The same computation in plain torch fp32 (matmuls, sigmoid) on the weights rounded to fp32; the top (softmax,
    loss) in fp32 too.  Returns (loss sum, gradient sum [P], logits) as fp64 numpy."""
    Wb = [(torch.tensor(W, dtype=torch.float32), torch.tensor(b, dtype=torch.float32))
          for W, b in unpack(np.asarray(theta, dtype=np.float64), layers)]
    acts = [torch.tensor(np.asarray(X), dtype=torch.float32)]
    for l, (W, b) in enumerate(Wb):
        z = acts[-1] @ W.T + b
        if l < len(Wb) - 1:
            acts.append(torch.sigmoid(z))
    yt = torch.tensor(np.asarray(y, dtype=np.int64))
    lse = torch.logsumexp(z, 1)
    loss = float((lse - z.gather(1, yt[:, None])[:, 0]).double().sum())
    D = torch.softmax(z, 1)
    D[torch.arange(len(yt)), yt] -= 1.0
    grads = [None] * len(Wb)
    for l in range(len(Wb) - 1, -1, -1):
        grads[l] = ((D.T @ acts[l]).double().numpy(), D.sum(0).double().numpy())
        if l > 0:
            D = (D @ Wb[l][0]) * acts[l] * (1.0 - acts[l])
    return loss, pack(grads), z.double().numpy()


def make_case(layers, n, seed=0, scale=1.0, dtype=np.float32):
    """(X, y, theta): continuous random rows, uniform labels, Spark-style uniform weights times ``scale``, rounded to
    fp32 so that the device op (defined at the fp32-rounded weights) and the reference share them exactly."""
    rng = np.random.default_rng(seed + 1000 * len(layers) + n)
    X = rng.normal(size=(n, layers[0])).astype(dtype)
    y = rng.integers(0, layers[-1], n).astype(np.int64)
    theta = np.zeros(num_params(layers))
    off = 0
    for i, o in zip(layers[:-1], layers[1:]):
        b = np.sqrt(6.0 / (i + o)) * scale
        theta[off:off + o * i] = rng.uniform(-b, b, o * i)
        theta[off + o * i:off + o * i + o] = rng.uniform(-0.5, 0.5, o) * scale
        off += o * i + o
    return X, y, theta.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(layers, n, seed=0, scale=1.0):
    """make_case with its reference and yardstick results, computed once and shared (treat as read-only):
    dict(X, y, theta, loss, grad, raw, prob, pred, y_loss, y_grad, y_raw)."""
    layers = list(layers)
    X, y, theta = make_case(layers, n, seed, scale)
    loss, grad = step(X, y, theta, layers)
    raw, prob, pred = predict(X, theta, layers)
    yl, yg, yz = yardstick(X, y, theta, layers)
    return dict(X=X, y=y, theta=theta, loss=loss, grad=grad, raw=raw, prob=prob, pred=pred, y_loss=yl, y_grad=yg,
                y_raw=yz)


def xor_data(n=400, seed=0, sigma=0.5):
    """Four Gaussian blobs at (+-2, +-2); the label is whether the signs differ."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, (n, 2)) * 2 - 1
    X = 2.0 * s + rng.normal(scale=sigma, size=(n, 2))
    return X, (s[:, 0] != s[:, 1]).astype(np.float64)


def three_class_data(n=600, d=4, seed=0):
    """Overlapping (non-separable) 3-class Gaussian data."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, n)
    mu = rng.normal(scale=1.0, size=(3, d))
    return mu[y] + rng.normal(scale=1.5, size=(n, d)), y.astype(np.float64)
