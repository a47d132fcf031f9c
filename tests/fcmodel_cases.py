"""The seeded cases of the FC box head's tests (no GPU import): tests/golden/make_golden_fcmodel.py runs the reference on them,
tests/test_fcmodel_host.py the float64 restatement (tests/fcmodel_ref.py), tests/test_gpu_fcmodel.py the kernels.

Every value is drawn in float32 (and widened exactly where float64 is wanted), so the float64 and float32 runs start from the
same numbers.  Running statistics, gamma and beta are random, not their initial 0 and 1.
"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name n input neurons blocks output leaky p seed")

# (N, input, neurons, blocks, output, leaky)
EVAL_CASES = [
    Case("head_n1", 1, 18, 128, 1, 5, False, 0.5, 101),          # the released head, one row
    Case("head_n17", 17, 18, 128, 1, 5, False, 0.5, 102),        # one row past a tile; K = 18 is no multiple of 4; 5 outputs in a 16 pad
    Case("w48_leaky", 33, 7, 48, 2, 3, True, 0.5, 103),          # three tiles; 48 = 16 * 3; two blocks reuse the in-place residual
    Case("no_block", 16, 18, 128, 0, 5, False, 0.5, 104),        # no block, an exact tile
    Case("defaults", 3, 32, 1024, 2, 64, False, 0.5, 105),       # the class defaults; the 128 KB LDS grant
]
TRAIN_CASES = [
    Case("train_n2", 2, 18, 128, 1, 5, False, 0.0, 201),         # the smallest legal batch, no dropout
    Case("train_n17", 17, 18, 128, 1, 5, False, 0.5, 202),
    Case("train_w48", 33, 7, 48, 2, 3, True, 0.5, 203),
]
BY_NAME = {c.name: c for c in EVAL_CASES + TRAIN_CASES}

# the quantities a bound is kept for; the pre-norm bias gradients are zero in exact arithmetic (the batch mean absorbs the bias)
TRAIN_KINDS = ("out", "grad_input", "grad_weight", "grad_bias", "grad_zero_bias", "grad_gamma", "grad_beta", "running_mean",
               "running_var")


def ctor_kwargs(c):
    return dict(num_neurons=c.neurons, num_blocks=c.blocks, p_dropout=c.p, leaky=c.leaky, input_size=c.input, output_size=c.output)


def layer_prefixes(blocks):
    """(Linear prefix, BatchNorm1d prefix) of the normalised layers in call order."""
    out = [("w1", "batch_norm1")]
    for b in range(blocks):
        out += [(f"res_blocks.{b}.w1", f"res_blocks.{b}.batch_norm1"), (f"res_blocks.{b}.w2", f"res_blocks.{b}.batch_norm2")]
    return out


def state_keys(c):
    """The state-dict keys and shapes in the module's order."""
    keys = []
    widths = [c.input] + [c.neurons] * (2 * c.blocks)
    for (lin, bn), k in zip(layer_prefixes(c.blocks), widths):
        keys += [(f"{lin}.weight", (c.neurons, k)), (f"{lin}.bias", (c.neurons,))]
        keys += [(f"{bn}.weight", (c.neurons,)), (f"{bn}.bias", (c.neurons,)), (f"{bn}.running_mean", (c.neurons,)),
                 (f"{bn}.running_var", (c.neurons,)), (f"{bn}.num_batches_tracked", ())]
    keys += [("w2.weight", (c.output, c.neurons)), ("w2.bias", (c.output,))]
    return keys


def state(c):
    """name -> float32 array (int64 for num_batches_tracked), in state-dict order."""
    r = np.random.default_rng(c.seed)
    sd = collections.OrderedDict()
    for name, shape in state_keys(c):
        leaf = name.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[name] = np.array(3, dtype=np.int64)
        elif leaf == "running_var":
            sd[name] = r.uniform(0.5, 2.0, shape).astype(np.float32)
        elif leaf == "running_mean":
            sd[name] = (0.5 * r.standard_normal(shape)).astype(np.float32)
        elif "batch_norm" in name and leaf == "weight":
            sd[name] = r.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == "bias":
            sd[name] = (0.2 * r.standard_normal(shape)).astype(np.float32)
        else:
            sd[name] = (r.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
    return sd


def inputs(c):
    """x [N, input] in 0 .. 1 (the coordinate head ends in a sigmoid), the functional's weights g [N, output] and, with
    p > 0, the keep masks uint8 [1 + 2 * blocks, N, neurons]."""
    r = np.random.default_rng(c.seed + 1000)
    x = r.uniform(0.0, 1.0, (c.n, c.input)).astype(np.float32)
    g = r.standard_normal((c.n, c.output)).astype(np.float32)
    masks = (r.random((1 + 2 * c.blocks, c.n, c.neurons)) >= c.p).astype(np.uint8) if c.p > 0 else None
    return x, g, masks


def vernier_cfg(grid=(16, 16, 24), **kw):
    """The local model's configuration as tests/test_gpu_parity.py builds it (its smallest grid, G1 of tests/golden_cases.py),
    with ``identity`` features."""
    import types
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=False, grid_resolution=list(grid), resolution=(64, 64),
                                x_range=(-1.0, 1.0), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = types.SimpleNamespace(output_channel=32, name="identity")
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def kind_of(name):
    """The bound's quantity for a parameter's gradient or a running statistic."""
    leaf = name.rsplit(".", 1)[1]
    if leaf in ("running_mean", "running_var"):
        return leaf
    if "batch_norm" in name:
        return "grad_gamma" if leaf == "weight" else "grad_beta"
    if leaf == "weight":
        return "grad_weight"
    return "grad_bias" if name == "w2.bias" else "grad_zero_bias"


def rel_err(got, want, scale=None):
    """max |got - want| over max |want| (or over ``scale``)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() if scale is None else scale))
