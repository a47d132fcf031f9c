"""Writes tests/golden/fcmodel_ref.npz: what the reference's own snvc/models/FCmodel.py computes on the cases of
tests/fcmodel_cases.py.

    python tests/golden/make_golden_fcmodel.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (its FCmodel.py is imported on the CPU, by path, not copied); the tests need only the file.
Inputs come from the cases' seeds, so the file holds results only:

    keys/<head|defaults>, shapes/<...>     the state-dict keys (in order) and shapes of get_fc_model() and of FCModel()
    out64/<case>, rep64/<case>             eval cases: forward and get_representation in float64
    e32/<case>                             [error of the float32 forward, of the float32 representation], each
                                           max |f32 - f64| / max |f64|
    train64/<case>/out                     training cases: the output in float64
    train64/<case>/grad/input, grad/<key>  the gradients of sum(out * g) for the input and every parameter
    train64/<case>/stat/<key>              the running statistics after the step
    train_e32/<case>                       the float32 run's error per quantity, in the order of fcmodel_cases.TRAIN_KINDS;
                                           per tensor max |f32 - f64| / max |f64|, the largest over the quantity's tensors.
                                           grad_zero_bias (the bias of a Linear in front of a BatchNorm: zero in exact
                                           arithmetic) is measured against max |f64 gradient of the same Linear's weight|.

With p > 0 each `dropout` attribute of the reference instance is replaced by one module that applies the case's masks in
call order.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")

import fcmodel_cases as FC  # noqa: E402

_spec = importlib.util.spec_from_file_location("ref_FCmodel", os.path.join(REF, "snvc", "models", "FCmodel.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


class GivenMasks(nn.Module):
    """Stands in for every nn.Dropout of one model: the k-th call applies the k-th mask."""

    def __init__(self, masks, p, dtype):
        super().__init__()
        self.masks, self.scale, self.calls = torch.from_numpy(masks).to(dtype), 1.0 / (1.0 - p), 0

    def forward(self, y):
        m = self.masks[self.calls]
        self.calls += 1
        return y * m * self.scale


def model_for(c, dtype):
    m = ref.FCModel(**FC.ctor_kwargs(c)).to(dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype if v.dtype != np.int64 else torch.int64) for k, v in FC.state(c).items()},
                      strict=True)
    return m


def eval_run(c, dtype):
    m = model_for(c, dtype).eval()
    x = torch.from_numpy(FC.inputs(c)[0]).to(dtype)
    with torch.no_grad():
        return m(x).double().numpy(), m.get_representation(x).double().numpy()


def train_run(c, dtype):
    m = model_for(c, dtype).train()
    x, g, masks = FC.inputs(c)
    if masks is not None:
        given = GivenMasks(masks, c.p, dtype)
        m.dropout = given
        for b in m.res_blocks:
            b.dropout = given
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = m(x)
    (out * torch.from_numpy(g).to(dtype)).sum().backward()
    grads = {"input": x.grad.double().numpy()}
    grads.update({k: p.grad.double().numpy() for k, p in m.named_parameters()})
    stats = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in m.state_dict().items()
             if k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")}
    return out.detach().double().numpy(), grads, stats


def train_e32(r64, r32):
    o64, g64, s64 = r64
    o32, g32, s32 = r32
    e = dict.fromkeys(FC.TRAIN_KINDS, 0.0)
    e["out"] = FC.rel_err(o32, o64)
    e["grad_input"] = FC.rel_err(g32["input"], g64["input"])
    for k in g64:
        if k == "input":
            continue
        kind = FC.kind_of(k)
        scale = np.abs(g64[k[:-4] + "weight"]).max() if kind == "grad_zero_bias" else None
        e[kind] = max(e[kind], FC.rel_err(g32[k], g64[k], scale))
    for k in s64:
        if not k.endswith("num_batches_tracked"):
            e[FC.kind_of(k)] = max(e[FC.kind_of(k)], FC.rel_err(s32[k], s64[k]))
    return np.array([e[k] for k in FC.TRAIN_KINDS])


def main():
    out = {}
    for tag, m in (("head", ref.get_fc_model()), ("defaults", ref.FCModel())):
        sd = m.state_dict()
        out[f"keys/{tag}"] = np.array(list(sd.keys()))
        out[f"shapes/{tag}"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    for c in FC.EVAL_CASES:
        o64, r64 = eval_run(c, torch.float64)
        o32, r32 = eval_run(c, torch.float32)
        out[f"out64/{c.name}"], out[f"rep64/{c.name}"] = o64, r64
        out[f"e32/{c.name}"] = np.array([FC.rel_err(o32, o64), FC.rel_err(r32, r64)])
        print(f"{c.name:12s} e32 out {out[f'e32/{c.name}'][0]:.3g} rep {out[f'e32/{c.name}'][1]:.3g}")
    for c in FC.TRAIN_CASES:
        r64, r32 = train_run(c, torch.float64), train_run(c, torch.float32)
        out[f"train64/{c.name}/out"] = r64[0]
        for k, v in r64[1].items():
            out[f"train64/{c.name}/grad/{k}"] = v
        for k, v in r64[2].items():
            out[f"train64/{c.name}/stat/{k}"] = v
        out[f"train_e32/{c.name}"] = train_e32(r64, r32)
        print(f"{c.name:12s} e32 " + " ".join(f"{k} {v:.3g}" for k, v in zip(FC.TRAIN_KINDS, out[f"train_e32/{c.name}"])))
    path = os.path.join(ROOT, "tests", "golden", "fcmodel_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
