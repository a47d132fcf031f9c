"""The 2D layer family under autograd (``_Conv2dNormActFn`` in snvc_amd/models/submodule.py, ``_FuseSumFn`` and the block / fusion
compositions of snvc_amd/models/hrnet.py): the case table and its float64 reference.  Importable without a GPU.

``ROWS``: one record per single layer.  The named rows pin one host decision of the backward each (see ``Row.pins``); the ``grid_*``
rows are the full product kind x norm x activation x residual at the smallest shapes, so that no combination the code can take is
left without a float64 comparison (tests/test_neck2d_backward_host.py asserts the product, less ``REFUSED``).  ``reference(row)``
evaluates the row with plain ``F.conv2d`` / ``F.conv_transpose2d`` / ``F.batch_norm`` / ``F.group_norm`` autograd on the float32 inputs
cast to double; nothing of the package is imported for it.  ``evaluate(row, data, torch.float32, gy)`` is the same expression in
float32: how far float32 arithmetic itself is from the reference.

ReLU is discontinuous: the upstream gradient is zeroed where the float64 pre-activation is within ``MASK`` of zero (the rule of
test_gpu_parity.test_layer_backward_vs_torch_autograd), at most ``MASK_CAP`` of a row's output elements.

``COMPOSITIONS``: HRNet blocks, one fusion row and ``_FuseSumFn`` alone, against float64 autograd of the same modules cast to double
on their torch route (``hrnet._block(b, x, False)`` / ``hrnet._module_torch``) on the CPU.  There an *internal* ReLU cannot be masked
through ``gy``: each row's seed is chosen so that every internal float64 pre-activation lies at least ``INTERNAL_MARGIN`` from zero.
"""
import itertools
from typing import FrozenSet, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

MASK = 1e-2                # |float64 pre-activation| below which a ReLU row's upstream gradient is zeroed
MASK_CAP = 0.02            # ... on at most this fraction of the row's output elements
INTERNAL_MARGIN = 1e-3     # compositions: every internal pre-activation at least this far from zero (1000x float32's error there)
F32_CAP = 2e-6             # torch's float32 CPU autograd of the same expression against the reference: a tenth of TIGHT

NORMS = ("bn_train", "bn_frozen", "gn", "bias", "none")
ACTS = ("none", "relu", "sigmoid")
RESIDUALS = ("none", "before", "after")
KINDS = (("conv", 1, 1), ("conv", 1, 2), ("conv", 3, 1), ("conv", 3, 2), ("deconv",), ("whole",))
ALL = frozenset(("x", "weight", "affine", "residual"))


class Row(NamedTuple):
    name: str
    kind: tuple                         # ("conv", k, stride) | ("deconv",) | ("whole",)
    n: int
    cin: int
    cout: int
    h: int
    w: int
    norm: str                           # one of NORMS
    act: str                            # one of ACTS
    residual: str                       # one of RESIDUALS
    needs: FrozenSet[str]               # which of x / weight / affine (norm affine or conv bias) / residual require a gradient
    seed: int
    pins: str = ""
    variant: Optional[str] = None       # name of the snvc_amd._lib conv_variant bits to force (forward and backward)
    groups: int = 32                    # GroupNorm groups
    transposed_input: bool = False      # fused_conv2d(..., transposed_input=True): the layer sees x.transpose(2, 3)
    same_as: Optional[str] = None       # a ``needs`` variant of that row: what it still returns equals that row's bit for bit


def _r(name, kind, n, cin, cout, h, w, norm, act, residual, seed, pins, needs=ALL, **kw):
    needs = frozenset(needs) - (frozenset(("residual",)) if residual == "none" else frozenset()) \
        - (frozenset(("affine",)) if norm == "none" else frozenset())
    return Row(name, kind, n, cin, cout, h, w, norm, act, residual, needs, seed, pins, **kw)


K1S1, K1S2, K3S1, K3S2, DECONV, WHOLE = KINDS

NAMED = [
    _r("k1s1_ragged_bn_relu_res", K1S1, 2, 12, 20, 5, 7, "bn_train", "relu", "before", 1,
       "widths off every channel chunk; the residual gradient is the masked one"),
    _r("k1s2_odd_bn_relu", K1S2, 2, 20, 12, 7, 9, "bn_train", "relu", "none", 2,
       "odd extents: scatter of the data gradient into [::2, ::2], x[::2, ::2] for the weight gradient"),
    _r("k1s2_frozen_res_no_act", K1S2, 2, 16, 32, 6, 8, "bn_frozen", "none", "before", 3,
       "the HRNet down-path form: gres must be gy itself"),
    _r("k3s1_ragged_bn_relu_res", K3S1, 2, 12, 28, 5, 7, "bn_train", "relu", "before", 4,
       "flipped and transposed data-gradient layer, ragged channels"),
    _r("k3s1_gn_relu_res_after", K3S1, 2, 32, 64, 6, 9, "gn", "relu", "after", 5,
       "GroupNorm coefficients per (sample, group); residual after the activation under training"),
    _r("k3s2_odd_bn_relu", K3S2, 2, 20, 36, 7, 9, "bn_train", "relu", "none", 6,
       "crop of the data gradient, pad of x for the weight gradient"),
    _r("k3s2_odd_w_frozen_res", K3S2, 2, 24, 40, 6, 13, "bn_frozen", "none", "before", 7, "odd in W only"),
    _r("k3s1_bias_sigmoid", K3S1, 2, 11, 8, 6, 4, "bias", "sigmoid", "none", 8, "gb = draw.sum, the sigmoid derivative"),
    _r("k3s1_bias_relu_res_after", K3S1, 2, 11, 8, 6, 4, "bias", "relu", "after", 9, "gb = draw.sum with a residual after the ReLU"),
    _r("k3s1_bias_sigmoid_res", K3S1, 2, 11, 8, 6, 4, "bias", "sigmoid", "before", 10, "the sigmoid derivative with a residual"),
    _r("k3s1_plain", K3S1, 2, 9, 27, 5, 6, "none", "none", "none", 11, "draw is gy"),
    _r("deconv_bn_relu_res", DECONV, 2, 36, 20, 4, 5, "bn_train", "relu", "before", 12,
       "the stride-2 data-gradient layer, roles swapped in the weight gradient"),
    _r("deconv_gn_relu_res_n1", DECONV, 1, 64, 32, 3, 5, "gn", "relu", "before", 13,
       "the transposed layer with GroupNorm and a residual, one sample"),
    _r("whole_bias_sigmoid", WHOLE, 3, 8, 6, 6, 4, "bias", "sigmoid", "none", 14, "the flattened 1x1 layer in both directions"),
    _r("k3s1_wino_bn_relu_res", K3S1, 2, 32, 32, 34, 36, "bn_train", "relu", "before", 15,
       "the depth-1 Winograd form taken by the forward and by the data-gradient layer", variant="ALGO_WINO_TILE_BIG"),
    _r("k3s1_frozen_relu_res", K3S1, 2, 12, 28, 5, 7, "bn_frozen", "relu", "before", 16, "the row the three needs variants are held to"),
    _r("k3s1_frozen_only_residual", K3S1, 2, 12, 28, 5, 7, "bn_frozen", "relu", "before", 16,
       "only the residual wants a gradient", needs=("residual",), same_as="k3s1_frozen_relu_res"),
    _r("k3s1_frozen_first_layer", K3S1, 2, 12, 28, 5, 7, "bn_frozen", "relu", "before", 16,
       "x does not want a gradient (a first layer)", needs=("weight", "affine", "residual"), same_as="k3s1_frozen_relu_res"),
    _r("k3s1_frozen_weights", K3S1, 2, 12, 28, 5, 7, "bn_frozen", "relu", "before", 16,
       "weights and affine frozen, x wants a gradient", needs=("x", "residual"), same_as="k3s1_frozen_relu_res"),
    _r("k3s1_transposed_input", K3S1, 2, 16, 16, 5, 7, "bn_train", "relu", "none", 17,
       "transposed_input under training: the fall-back copy computes conv(x.transpose(2, 3))", transposed_input=True),
]

# what the code refuses, by name; tests/test_gpu_neck2d_backward.py asserts the NotImplementedError of each
REFUSED = {
    "bias_with_norm": "a conv bias together with a norm, under training",
    "dilated_training": "a dilated Conv2d under training",
    "out_training": "an `out=` slice under training",
    "deconv_bias": "fused_deconv2d takes ConvTranspose2d(bias=False) only",
}
# fused_deconv2d has neither a sigmoid nor a residual after the activation: the code cannot take these
DECONV_ACTS, DECONV_RESIDUALS = ("none", "relu"), ("none", "before")

_GRID_SHAPE = {K1S1: (2, 5, 8, 5, 6), K1S2: (2, 5, 8, 9, 11), K3S1: (2, 5, 8, 5, 6), K3S2: (2, 5, 8, 9, 11),
               DECONV: (2, 5, 8, 3, 4), WHOLE: (8, 5, 8, 3, 4)}
# grid rows whose first seed masks more than MASK_CAP of their (few) output elements take the next one that does not
_GRID_SEED = {"grid_whole_bn_frozen_relu_res_none": 2237}       # 64 output elements: one masked element is 1.6 %, two are not allowed


def _kind_name(kind):
    return f"k{kind[1]}s{kind[2]}" if kind[0] == "conv" else kind[0]


def can_take(kind, norm, act, residual) -> bool:
    """The combinations of the full product that the code can take."""
    if kind == DECONV:
        return norm != "bias" and act in DECONV_ACTS and residual in DECONV_RESIDUALS
    return True


def _grid():
    rows = []
    for i, (kind, norm, act, residual) in enumerate(itertools.product(KINDS, NORMS, ACTS, RESIDUALS)):
        if not can_take(kind, norm, act, residual):
            continue
        name = f"grid_{_kind_name(kind)}_{norm}_{act}_res_{residual}"
        rows.append(_r(name, kind, *_GRID_SHAPE[kind], norm, act, residual, _GRID_SEED.get(name, 1000 + i), "the full product",
                       groups=1 if kind == WHOLE else 4))      # a group of two values has a gradient of pure cancellation
    return rows


ROWS = NAMED + _grid()
BY_NAME = {r.name: r for r in ROWS}


# ------------------------------------------------------------------------------------------------------------------ one layer
def weight_shape(row: Row):
    if row.kind == DECONV:
        return (row.cin, row.cout, 3, 3)
    if row.kind == WHOLE:
        return (row.cout, row.cin, row.h, row.w)
    return (row.cout, row.cin, row.kind[1], row.kind[1])


def seen_extent(row: Row):
    """(H, W) as the convolution sees them."""
    return (row.w, row.h) if row.transposed_input else (row.h, row.w)


def out_shape(row: Row):
    h, w = seen_extent(row)
    if row.kind == DECONV:
        return (row.n, row.cout, 2 * h, 2 * w)
    if row.kind == WHOLE:
        return (row.n, row.cout, 1, 1)
    k, s = row.kind[1], row.kind[2]
    p = (k - 1) // 2
    return (row.n, row.cout, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1)


def build(row: Row) -> dict:
    """The row's float32 inputs on the CPU, from its seed alone (a ``needs`` variant of a row draws the same)."""
    r = np.random.default_rng(7000 + row.seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    ws = weight_shape(row)
    fan_in = row.cin * ws[2] * ws[3] / (4 if row.kind == DECONV else 1)
    d = dict(x=f(r.standard_normal((row.n, row.cin, row.h, row.w))),
             weight=f(r.standard_normal(ws) / np.sqrt(fan_in)),
             gamma=f(r.uniform(0.5, 1.5, row.cout)), beta=f(r.uniform(-0.3, 0.3, row.cout)),
             bias=f(r.uniform(-0.5, 0.5, row.cout)),
             running_mean=f(0.3 * r.standard_normal(row.cout)), running_var=f(r.uniform(0.5, 1.5, row.cout)),
             residual=f(r.standard_normal(out_shape(row))), gy=f(r.standard_normal(out_shape(row))))
    return d


def _conv(row: Row, x, w, b):
    if row.transposed_input:
        x = x.transpose(2, 3)
    if row.kind == DECONV:
        return F.conv_transpose2d(x, w, None, 2, 1, 1)
    if row.kind == WHOLE:
        return F.conv2d(x, w, b)
    k, s = row.kind[1], row.kind[2]
    return F.conv2d(x, w, b, s, (k - 1) // 2)


def evaluate(row: Row, data: dict, dtype, gy=None) -> dict:
    """The row in ``dtype`` on the CPU with torch's own operators and autograd.  ``gy`` None: forward only (y, pre-activation, running
    statistics); else every gradient the row requests as well."""
    t = {k: v.to(dtype).clone() for k, v in data.items()}
    for k in ("x", "weight", "gamma", "beta", "bias", "residual"):
        t[k].requires_grad_(True)
    v = _conv(row, t["x"], t["weight"], t["bias"] if row.norm == "bias" else None)
    out = {}
    if row.norm in ("bn_train", "bn_frozen"):
        rm, rv = t["running_mean"], t["running_var"]
        v = F.batch_norm(v, rm, rv, t["gamma"], t["beta"], row.norm == "bn_train", 0.1, 1e-5)
        out["running_mean"], out["running_var"] = rm, rv
    elif row.norm == "gn":
        v = F.group_norm(v, row.groups, t["gamma"], t["beta"], 1e-5)
    if row.residual == "before":
        v = v + t["residual"]
    out["pre"] = v.detach()
    y = {"none": lambda a: a, "relu": torch.relu, "sigmoid": torch.sigmoid}[row.act](v)
    if row.residual == "after":
        y = y + t["residual"]
    out["y"] = y.detach()
    if gy is not None:
        y.backward(gy.to(dtype))
        out["dx"], out["dw"], out["dres"] = t["x"].grad, t["weight"].grad, t["residual"].grad
        if row.norm in ("bn_train", "bn_frozen", "gn"):
            out["dgamma"], out["dbeta"] = t["gamma"].grad, t["beta"].grad
        if row.norm == "bias":
            out["dbias"] = t["bias"].grad
    return out


def requested(row: Row):
    """The gradients the row asks for, by the names ``reference`` uses."""
    names = []
    if "x" in row.needs:
        names.append("dx")
    if "weight" in row.needs:
        names.append("dw")
    if "affine" in row.needs:
        names += ["dbias"] if row.norm == "bias" else ["dgamma", "dbeta"]
    if "residual" in row.needs:
        names.append("dres")
    return names


def residual_gradient_is_gy(row: Row) -> bool:
    """A residual behind no activation, or added after it: its gradient is the upstream gradient, bit for bit."""
    return row.residual == "after" or (row.residual == "before" and row.act == "none")


def masked_gy(row: Row, data: dict, pre64):
    """(gy with the elements next to a ReLU's kink zeroed, the fraction zeroed)."""
    if row.act != "relu":
        return data["gy"], 0.0
    near = pre64.abs() < MASK
    return data["gy"].masked_fill(near, 0.0), float(near.double().mean())


def reference(row: Row, data: Optional[dict] = None) -> dict:
    """y, every requested gradient and (bn_train) the updated running statistics in float64; also ``gy`` (float32, masked: what the
    route under test must be given) and ``masked`` (the fraction of it that was zeroed)."""
    data = build(row) if data is None else data
    gy, frac = masked_gy(row, data, evaluate(row, data, torch.float64)["pre"])
    full = evaluate(row, data, torch.float64, gy)
    out = {k: full[k] for k in ["y"] + requested(row)}
    if row.norm == "bn_train":
        out["running_mean"], out["running_var"] = full["running_mean"], full["running_var"]
    out["gy"], out["masked"] = gy, frac
    return out


def rel_err(a, b) -> float:
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# --------------------------------------------------------------------------------------------------------------- compositions
class Composition(NamedTuple):
    name: str
    what: str                           # "bottleneck" | "basic" | "fuse_row" | "fuse_sum"
    shapes: Tuple[tuple, ...]           # of the inputs
    seed: int
    layers: int                         # layers that go through _Conv2dNormActFn on the HIP route
    factors: tuple = ()                 # fuse_sum: the terms' up-sampling factors
    frozen: Optional[int] = None        # fuse_sum: the one term that does not require a gradient
    pins: str = ""


FUSE_WIDTHS, FUSE_ROW = (8, 12, 20), 2

COMPOSITIONS = [
    Composition("bottleneck_12_5_downsample", "bottleneck", ((2, 12, 4, 6),), 2, 4, pins="Bottleneck(12, 5) with a 1x1 + BN downsample, train mode"),
    Composition("basic_12_12", "basic", ((2, 12, 4, 6),), 1, 2, pins="x feeds conv1 and the residual: two gradients meet"),
    Composition("fuse_row_2_of_3", "fuse_row", ((1, 8, 16, 16), (1, 12, 8, 8), (1, 20, 4, 4)), 0, 7,
                pins="a chain of two stride-2 layers, the accumulating residual=part and _FuseSumFn"),
] + [Composition(f"fuse_sum_{'_'.join(map(str, fs))}_frozen_{i}", "fuse_sum",
                 tuple((n, c, h // f, w // f) for f in fs), 0, 0, fs, i, "one term of _FuseSumFn does not require a gradient")
     for fs, (n, c, h, w) in (((1, 2, 4), (1, 3, 8, 8)), ((1, 1, 2, 4), (2, 4, 8, 12))) for i in range(len(fs))]
COMP_BY_NAME = {c.name: c for c in COMPOSITIONS}


def init_module(m: torch.nn.Module, seed: int) -> torch.nn.Module:
    """Seeded parameters and running statistics: convolutions N(0, 1 / fan-in), norm affines and statistics away from 1 and 0."""
    r = np.random.default_rng(9000 + seed)
    with torch.no_grad():
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() == 4:
                v = r.standard_normal(tuple(t.shape)) / np.sqrt(t.shape[1] * t.shape[2] * t.shape[3])
            elif name.endswith("running_var"):
                v = r.uniform(0.5, 1.5, tuple(t.shape))
            elif name.endswith("running_mean"):
                v = 0.3 * r.standard_normal(tuple(t.shape))
            elif name.endswith("weight"):
                v = r.uniform(0.5, 1.5, tuple(t.shape))
            else:
                v = r.uniform(-0.3, 0.3, tuple(t.shape))
            t.copy_(torch.from_numpy(v.astype(np.float32)))
    return m


def make_module(c: Composition) -> Optional[torch.nn.Module]:
    """The composition's module (float32, CPU, train mode) with its seeded state; None for ``_FuseSumFn`` alone."""
    from snvc_amd.models import hrnet as H
    from snvc_amd.models import submodule as S
    if c.what == "bottleneck":
        down = torch.nn.Sequential(torch.nn.Conv2d(12, 20, kernel_size=1, stride=1, bias=False), H._bn(20))
        m = H.Bottleneck(12, 5, 1, down)
    elif c.what == "basic":
        m = S.BasicBlock2d(12, 12)
    elif c.what == "fuse_row":
        m = H.HighResolutionModule(len(FUSE_WIDTHS), H.BasicBlock, [1] * len(FUSE_WIDTHS), list(FUSE_WIDTHS), list(FUSE_WIDTHS), "SUM")
        m.branches = torch.nn.ModuleList([torch.nn.Sequential() for _ in FUSE_WIDTHS])      # the fusion alone: every branch the identity
    else:
        return None
    return init_module(m, c.seed).train()


def comp_inputs(c: Composition):
    """(inputs, upstream gradient before masking): float32, CPU."""
    r = np.random.default_rng(9500 + c.seed + 17 * len(c.shapes) + sum(c.factors))
    xs = [torch.from_numpy(r.standard_normal(s).astype(np.float32)) for s in c.shapes]
    gshape = c.shapes[FUSE_ROW] if c.what == "fuse_row" else ((c.shapes[0][0], 20) + c.shapes[0][2:] if c.what == "bottleneck" else c.shapes[0])
    return xs, torch.from_numpy(r.standard_normal(gshape).astype(np.float32))


def _torch_fuse(terms, factors):
    y = None
    for t, f in zip(terms, factors):
        t = F.interpolate(t, scale_factor=f, mode="nearest") if f > 1 else t
        y = t if y is None else y + t
    return y


def comp_forward_torch(c: Composition, m, xs):
    """The composition on its torch route: (outputs, the one that the loss takes, internal pre-activations, the last pre-activation)."""
    from snvc_amd.models import hrnet as H
    seen, hooks = {}, []
    if c.what == "fuse_sum":
        pre = _torch_fuse(xs, c.factors)
        return [torch.relu(pre)], 0, [], pre.detach()
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            hooks.append(mod.register_forward_hook(lambda _m, _i, o, name=name: seen.__setitem__(name, o.detach())))
        if isinstance(mod, torch.nn.ReLU):
            hooks.append(mod.register_forward_pre_hook(lambda _m, i, name=name: seen.setdefault("relu:" + name, []).append(i[0].detach())))
    try:
        if c.what == "fuse_row":
            outs = H._module_torch(m, list(xs))
            internal = [t for k, v in seen.items() if k.startswith(f"relu:fuse_layers.{FUSE_ROW}.") for t in v]
            assert len(internal) == 1 and len(seen["relu:relu"]) == len(FUSE_WIDTHS)
            return outs, FUSE_ROW, internal, seen["relu:relu"][FUSE_ROW]
        y = H._block(m, xs[0], False)
        last = "bn3" if c.what == "bottleneck" else "bn2"
        internal = [seen[k] for k in ("bn1", "bn2", "bn3") if k in seen and k != last]
        res = seen["downsample.1"] if m.downsample is not None else xs[0].detach()
        return [y], 0, internal, seen[last] + res
    finally:
        for h in hooks:
            h.remove()


def comp_evaluate(c: Composition, dtype, gy=None) -> dict:
    """The composition in ``dtype`` on the CPU torch route: outputs, pre-activations, and with ``gy`` the gradients of the inputs
    (None for a frozen one), of every parameter by name, and the running statistics afterwards."""
    m = make_module(c)
    xs0, _ = comp_inputs(c)
    if m is not None:
        m = m.to(dtype)
    xs = [x.to(dtype).requires_grad_(i != c.frozen) for i, x in enumerate(xs0)]
    outs, which, internal, last = comp_forward_torch(c, m, xs)
    out = dict(ys=[o.detach() for o in outs], which=which, internal=internal, last=last)
    if gy is not None:
        outs[which].backward(gy.to(dtype))
        out["dx"] = [x.grad for x in xs]
        if m is not None:
            out["params"] = {k: p.grad for k, p in m.named_parameters()}
            out["stats"] = {k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return out


def comp_reference(c: Composition) -> dict:
    """``comp_evaluate`` in float64 under the masked upstream gradient ``gy`` (float32, returned with it)."""
    fwd = comp_evaluate(c, torch.float64)
    _, gy = comp_inputs(c)
    near = fwd["last"].abs() < MASK
    gy = gy.masked_fill(near, 0.0)
    out = comp_evaluate(c, torch.float64, gy)
    out["gy"], out["masked"] = gy, float(near.double().mean())
    return out
