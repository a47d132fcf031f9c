"""A float64 numpy restatement of the FC box head (reference FCmodel.py): forward in eval and in train mode with given keep
masks, the backward of a linear functional of the output, and the running-statistics update.  tests/test_fcmodel_host.py
holds it to the reference's own float64 results (tests/golden/fcmodel_ref.npz) and to torch's autograd.
"""
import collections

import numpy as np

from fcmodel_cases import layer_prefixes

EPS, MOMENTUM, LEAKY_SLOPE = 1e-5, 0.1, 0.01      # nn.BatchNorm1d's and nn.LeakyReLU's defaults


def _f64(sd):
    return {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}


def forward(sd, x, blocks, leaky=False, train=False, masks=None, p=0.0, representation=False):
    """-> (output, cache).  ``masks``: uint8 [1 + 2 * blocks, N, neurons] keep masks in call order, or None (no dropout).
    In train mode the batch statistics normalise; the cache holds what ``backward`` and ``updated_stats`` need."""
    sd, cur = _f64(sd), np.asarray(x, dtype=np.float64)
    slope = LEAKY_SLOPE if leaky else 0.0
    cache = {"layers": [], "blocks": blocks, "slope": slope, "representation": representation, "x": cur}
    block_in = None
    for i, (lin, bn) in enumerate(layer_prefixes(blocks)):
        if i % 2 == 1:
            block_in = cur
        z = cur @ sd[f"{lin}.weight"].T + sd[f"{lin}.bias"]
        if train:
            mean, var = z.mean(axis=0), z.var(axis=0)
        else:
            mean, var = sd[f"{bn}.running_mean"], sd[f"{bn}.running_var"]
        istd = 1.0 / np.sqrt(var + EPS)
        xhat = (z - mean) * istd
        y = xhat * sd[f"{bn}.weight"] + sd[f"{bn}.bias"]
        positive = y > 0
        a = np.where(positive, y, slope * y)
        keep = None
        if train and masks is not None:
            keep = masks[i].astype(np.float64) / (1.0 - p)
            a = a * keep
        out = a + block_in if (i > 0 and i % 2 == 0) else a
        cache["layers"].append(dict(lin=lin, bn=bn, inp=cur, xhat=xhat, istd=istd, positive=positive, keep=keep, mean=mean, var=var,
                                    gamma=sd[f"{bn}.weight"], weight=sd[f"{lin}.weight"]))
        cur = out
    cache["rep"] = cur
    cache["w2"] = sd["w2.weight"]
    if representation:
        return cur, cache
    return cur @ sd["w2.weight"].T + sd["w2.bias"], cache


def backward(cache, gout):
    """Gradients of sum(output * gout) after a train-mode ``forward``: (grad of x, {parameter name: grad})."""
    gout = np.asarray(gout, dtype=np.float64)
    grads = collections.OrderedDict()
    if cache["representation"]:
        dy = gout
    else:
        grads["w2.weight"] = gout.T @ cache["rep"]
        grads["w2.bias"] = gout.sum(axis=0)
        dy = gout @ cache["w2"]
    block_grad = None
    for i in range(len(cache["layers"]) - 1, -1, -1):
        L = cache["layers"][i]
        if i > 0 and i % 2 == 0:
            block_grad = dy
        g = dy if L["keep"] is None else dy * L["keep"]
        g = np.where(L["positive"], g, cache["slope"] * g)
        dbeta, dgamma = g.sum(axis=0), (g * L["xhat"]).sum(axis=0)
        n = g.shape[0]
        dz = L["gamma"] * L["istd"] * (g - dbeta / n - L["xhat"] * dgamma / n)
        grads[f"{L['lin']}.weight"] = dz.T @ L["inp"]
        grads[f"{L['lin']}.bias"] = dz.sum(axis=0)
        grads[f"{L['bn']}.weight"] = dgamma
        grads[f"{L['bn']}.bias"] = dbeta
        dy = dz @ L["weight"]
        if i % 2 == 1:
            dy = dy + block_grad
    return dy, grads


def updated_stats(sd, cache):
    """The running statistics after the train-mode step of ``cache``: {name: value}."""
    out = collections.OrderedDict()
    for L in cache["layers"]:
        n = L["inp"].shape[0]
        bn = L["bn"]
        out[f"{bn}.running_mean"] = (1 - MOMENTUM) * np.asarray(sd[f"{bn}.running_mean"], dtype=np.float64) + MOMENTUM * L["mean"]
        out[f"{bn}.running_var"] = (1 - MOMENTUM) * np.asarray(sd[f"{bn}.running_var"], dtype=np.float64) + MOMENTUM * L["var"] * n / (n - 1)
        out[f"{bn}.num_batches_tracked"] = np.asarray(sd[f"{bn}.num_batches_tracked"]) + 1
    return out
