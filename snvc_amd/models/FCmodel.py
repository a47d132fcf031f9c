"""Drop-in for ``snvc.models.FCmodel``: the residual MLP that ``VernierScale`` uses as its box head (``use_bbox_head``).

Constructor arguments and defaults, module tree, attribute names and state-dict keys equal the reference's (FCmodel.py), so a
reference checkpoint loads with ``strict=True``; as there, ``FCModel`` does not hand ``kaiming`` down to its blocks.  What
changes is how ``FCModel.forward`` / ``get_representation`` execute (``csrc/fc_head.hip``, C ABI ``include/snvc_fc.h``, DESIGN
"FC box head"):

  module state                                            route
  ------------------------------------------------------- -------------------------------------------------------------
  every BatchNorm1d in eval, no gradient needed            ONE launch for the whole network: 16 rows per workgroup, the
                                                           activations in LDS from input to output, the weights streamed
                                                           from one packed buffer with the norms folded in
  every BatchNorm1d in train mode (with or without grad)   one launch per Linear + BatchNorm1d + activation + dropout layer
                                                           (batch statistics, running statistics and the residual add in
                                                           the neuron slab's owner); backward two launches per layer
  eval-mode norms under autograd, a mix of modes           the modules' torch forward on the GPU

The HIP routes serve a contiguous float32 GPU input ``[N, input_size]`` when every norm is a ``BatchNorm1d``,
``num_neurons % 16 == 0`` and ``num_neurons``, ``input_size`` and ``output_size`` are at most 1024; everything else (other
dtypes, other widths) runs the same modules' torch forward on the GPU.  ``FC_HIP[0] = False`` forces that torch route (the
same-module baseline of the tests and of tools/bench_fc.py).  Every decision is counted in ``submodule._ROUTES`` as "fc_hip"
or "fc_torch".  There is no CPU path: a CPU input raises.

Dropout in the training route: the module draws every layer's keep mask itself with torch on the device, from torch's current
CUDA generator (``_draw_masks``), so ``torch.manual_seed`` reproduces a step; the kernels only apply the masks.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _fc
from .._derived import derived
from .._lib import check
from ..ops import _written
from .submodule import _ROUTES, plan_for

FC_HIP = [True]      # False: FCModel takes the modules' torch forward


def _activation(leaky):
    return nn.LeakyReLU(inplace=True) if leaky else nn.ReLU(inplace=True)


class ResidualBlock(nn.Module):
    """x + (Linear, BatchNorm1d, activation, Dropout) twice (reference FCmodel.py:7-41)."""

    def __init__(self, num_neurons, p_dropout=0.5, kaiming=False, leaky=False):
        super().__init__()
        self.num_neurons = num_neurons
        self.leaky = leaky
        self.p_dropout = p_dropout
        self.relu = _activation(leaky)
        self.dropout = nn.Dropout(p_dropout)
        self.w1 = nn.Linear(num_neurons, num_neurons)
        self.batch_norm1 = nn.BatchNorm1d(num_neurons)
        self.w2 = nn.Linear(num_neurons, num_neurons)
        self.batch_norm2 = nn.BatchNorm1d(num_neurons)
        if kaiming:
            nn.init.kaiming_normal_(self.w1.weight.data)
            nn.init.kaiming_normal_(self.w2.weight.data)

    def forward(self, x):
        """The torch forward; ``FCModel`` runs its blocks inside its own kernels when it takes a HIP route."""
        y = self.dropout(self.relu(self.batch_norm1(self.w1(x))))
        y = self.dropout(self.relu(self.batch_norm2(self.w2(y))))
        return x + y


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _TrainFn(torch.autograd.Function):
    """One training call of the whole network on the per-layer kernels.  Inputs: x, then per normalised layer (weight, bias,
    gamma, beta), then the last Linear's (weight, bias); gradients go to every one of them."""

    @staticmethod
    def forward(ctx, model, masks, representation, x, *params):
        out, saved = model._train_forward(x, masks, representation, params, keep=True)
        ctx.model, ctx.masks, ctx.representation, ctx.n_params = model, masks, representation, len(params)
        ctx.save_for_backward(x, *params, *saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        params, saved = rest[:ctx.n_params], rest[ctx.n_params:]
        grads = ctx.model._train_backward(grad.contiguous(), x, ctx.masks, ctx.representation, params, saved)
        return (None, None, None) + tuple(grads)


class FCModel(nn.Module):
    """Linear + BatchNorm1d + activation + Dropout, ``num_blocks`` residual blocks, Linear (reference FCmodel.py:43-97)."""

    def __init__(self, num_neurons=1024, num_blocks=2, p_dropout=0.5, kaiming=False, leaky=False, input_size=32, output_size=64):
        super().__init__()
        self.num_neurons = num_neurons
        self.p_dropout = p_dropout
        self.num_blocks = num_blocks
        self.leaky = leaky
        self.input_size = input_size
        self.output_size = output_size
        self.w1 = nn.Linear(input_size, num_neurons)
        self.batch_norm1 = nn.BatchNorm1d(num_neurons)
        # the blocks do not get `kaiming`: the reference does not pass it down either
        self.res_blocks = nn.ModuleList([ResidualBlock(num_neurons=num_neurons, p_dropout=p_dropout, leaky=leaky)
                                         for _ in range(num_blocks)])
        self.w2 = nn.Linear(num_neurons, output_size)
        self.relu = _activation(leaky)
        self.dropout = nn.Dropout(p_dropout)
        if kaiming:
            nn.init.kaiming_normal_(self.w1.weight.data)
            nn.init.kaiming_normal_(self.w2.weight.data)

    # ------------------------------------------------------------------ structure
    def _norm_layers(self):
        """(Linear, norm, activation, dropout) of every normalised layer, in call order."""
        layers = [(self.w1, self.batch_norm1, self.relu, self.dropout)]
        for b in self.res_blocks:
            layers += [(b.w1, b.batch_norm1, b.relu, b.dropout), (b.w2, b.batch_norm2, b.relu, b.dropout)]
        return layers

    def _sources(self):
        """Every tensor the packed eval buffer is derived from."""
        src = []
        for lin, bn, _, _ in self._norm_layers():
            src += [lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return tuple(src) + (self.w2.weight, self.w2.bias)

    def _route(self, x):
        """"eval" / "train" (the HIP routes) or "torch"; counted in ``_ROUTES``."""
        if not x.is_cuda:
            raise RuntimeError("FCModel input must be a GPU tensor: Not implemented on the CPU")
        layers = self._norm_layers()
        route = "torch"
        w, slope = self.num_neurons, 0.01 if self.leaky else None
        shapes = [(w, self.input_size)] + [(w, w)] * (len(layers) - 1)

        def act_ok(a):
            return (isinstance(a, nn.LeakyReLU) and a.negative_slope == slope) if self.leaky else isinstance(a, nn.ReLU)
        ok = (FC_HIP[0] and x.dtype == torch.float32 and x.dim() == 2 and x.size(1) == self.input_size and x.is_contiguous()
              and len(layers) == 1 + 2 * self.num_blocks and w % 16 == 0
              and max(w, self.input_size, self.output_size) <= _fc.MAX_WIDTH
              and all(type(bn) is nn.BatchNorm1d and bn.affine and bn.track_running_stats and bn.momentum is not None
                      and isinstance(lin, nn.Linear) and lin.bias is not None and tuple(lin.weight.shape) == shape
                      and isinstance(drop, nn.Dropout) and drop.p == self.p_dropout and act_ok(a)
                      for (lin, bn, a, drop), shape in zip(layers, shapes))
              and isinstance(self.w2, nn.Linear) and self.w2.bias is not None
              and tuple(self.w2.weight.shape) == (self.output_size, w) and 0.0 <= self.p_dropout < 1.0
              and all(t.dtype == torch.float32 and t.device == x.device and t.is_contiguous() for t in self._sources()))
        if ok:
            modes = {bn.training for _, bn, _, _ in layers} | {drop.training for _, _, _, drop in layers}
            needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
            if modes == {True}:
                route = "train"
            elif modes == {False} and not needs_grad:
                route = "eval"
        _ROUTES["fc_torch" if route == "torch" else "fc_hip"] += 1
        return route

    # ------------------------------------------------------------------ the torch route
    def _torch_representation(self, x):
        y = self.dropout(self.relu(self.batch_norm1(self.w1(x))))
        for block in self.res_blocks:
            y = block(y)
        return y

    # ------------------------------------------------------------------ eval: one launch
    def _packed(self, device):
        """Every layer's weights in the eval kernel's layout (include/snvc_fc.h), BatchNorm folded: per neuron the scale
        gamma / sqrt(running_var + eps) goes into the weight row, the shift absorbs the Linear bias.  Folded in float64 and
        rounded once."""
        def slabs(weight, scale, shift):
            m, k = weight.shape
            kp, mp = (k + 3) // 4 * 4, (m + 15) // 16 * 16
            full = torch.zeros((mp, kp), dtype=torch.float64, device=device)
            full[:m, :k] = weight.detach().double() * scale[:, None]
            sh = torch.zeros(mp, dtype=torch.float64, device=device)
            sh[:m] = shift
            # [mp][kp] -> slabs of 16 neurons, each [kp][16]
            return [full.view(mp // 16, 16, kp).permute(0, 2, 1).reshape(-1).float(), sh.float()]

        def build():
            parts = []
            for lin, bn, _, _ in self._norm_layers():
                scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
                shift = (lin.bias.detach().double() - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
                parts += slabs(lin.weight, scale, shift)
            parts += slabs(self.w2.weight, torch.ones(self.output_size, dtype=torch.float64, device=device), self.w2.bias.detach().double())
            packed = torch.cat(parts).contiguous()
            want = _fc.lib().snvc_fc_packed_floats(self.input_size, self.num_neurons, self.num_blocks, self.output_size)
            assert packed.numel() == want, (packed.numel(), want)
            return packed
        return derived(plan_for(self, "", device), "fc_packed", self._sources(), build)

    def _eval_forward(self, x, representation):
        n = x.size(0)
        out = torch.empty((n, self.num_neurons if representation else self.output_size), dtype=torch.float32, device=x.device)
        packed = self._packed(x.device)
        with torch.cuda.device(x.device):
            check(_fc.lib().snvc_fc_eval_forward(_p(x), _p(packed), _p(out), n, self.input_size, self.num_neurons, self.num_blocks,
                                                 self.output_size, int(bool(self.leaky)), int(representation), _stream(x)),
                  "snvc_fc_eval_forward")
        return out

    # ------------------------------------------------------------------ training: one launch per layer
    def _draw_masks(self, n, device):
        """The keep masks of one training call, uint8 [1 + 2 * num_blocks, n, num_neurons] in call order (1 = kept), drawn
        from torch's current CUDA generator; None when p_dropout == 0.  Tests override this to supply known masks."""
        if self.p_dropout == 0:
            return None
        shape = (1 + 2 * self.num_blocks, n, self.num_neurons)
        return (torch.rand(shape, dtype=torch.float32, device=device) >= self.p_dropout).to(torch.uint8)

    def _train_params(self):
        params = []
        for lin, bn, _, _ in self._norm_layers():
            params += [lin.weight, lin.bias, bn.weight, bn.bias]
        return params + [self.w2.weight, self.w2.bias]

    def _train_forward(self, x, masks, representation, params, keep):
        """The layers in call order.  Returns (output, saved): per normalised layer its input is the previous output, and
        (xhat, mean, istd, out) are kept for the backward when ``keep``."""
        L = _fc.lib()
        n, w, dev = x.size(0), self.num_neurons, x.device
        layers = self._norm_layers()
        keep_scale = 1.0 / (1.0 - self.p_dropout)
        saved, cur, block_in = [], x, None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        with torch.cuda.device(dev):
            stream = _stream(x)
            for i, (lin, bn, _, _) in enumerate(layers):
                weight, bias, gamma, beta = params[4 * i:4 * i + 4]
                first_of_block, second_of_block = i % 2 == 1, i > 0 and i % 2 == 0
                if first_of_block:
                    block_in = cur
                xhat, mean, istd, out = new(n, w), new(w), new(w), new(n, w)
                check(L.snvc_fc_train_layer_forward(
                    _p(cur), _p(weight), _p(bias), _p(gamma), _p(beta), _p(bn.running_mean), _p(bn.running_var),
                    _p(bn.num_batches_tracked), _p(masks[i] if masks is not None else None),
                    _p(block_in if second_of_block else None), _p(xhat), _p(mean), _p(istd), _p(out), n, cur.size(1), w,
                    float(bn.eps), float(bn.momentum), keep_scale, int(bool(self.leaky)), stream), "snvc_fc_train_layer_forward")
                _written(bn.running_mean, bn.running_var, bn.num_batches_tracked)
                if keep:
                    saved += [xhat, istd, out]
                cur = out
            if not representation:
                weight, bias = params[-2:]
                out = new(n, self.output_size)
                check(L.snvc_fc_train_layer_forward(_p(cur), _p(weight), _p(bias), *([_p(None)] * 10), _p(out), n, w, self.output_size,
                                                    0.0, 0.0, 1.0, 0, stream), "snvc_fc_train_layer_forward")
                cur = out
        return cur, saved

    def _train_backward(self, grad, x, masks, representation, params, saved):
        """Gradients of x and of every entry of ``params``, in that order."""
        L = _fc.lib()
        n, w, dev = x.size(0), self.num_neurons, x.device
        layers = self._norm_layers()
        keep_scale = 1.0 / (1.0 - self.p_dropout)
        leaky = int(bool(self.leaky))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        grads = [None] * len(params)
        outs = [saved[3 * i + 2] for i in range(len(layers))]
        with torch.cuda.device(dev):
            stream = _stream(x)
            if representation:
                dy = grad
                grads[-2], grads[-1] = torch.zeros_like(params[-2]), torch.zeros_like(params[-1])
            else:
                weight = params[-2]
                grads[-2], grads[-1], dy = new(self.output_size, w), new(self.output_size), new(n, w)
                check(L.snvc_fc_train_layer_backward_params(_p(grad), _p(outs[-1]), *([_p(None)] * 5), _p(None), _p(None), _p(None),
                                                            _p(grads[-2]), _p(grads[-1]), n, w, self.output_size, 1.0, 0, stream),
                      "snvc_fc_train_layer_backward_params")
                check(L.snvc_fc_train_layer_backward_input(_p(grad), _p(weight), _p(None), _p(dy), n, w, self.output_size, stream),
                      "snvc_fc_train_layer_backward_input")
            block_grad = None      # the gradient of a block's output, which also reaches the block's input
            for i in range(len(layers) - 1, -1, -1):
                weight, bias, gamma, beta = params[4 * i:4 * i + 4]
                xhat, istd = saved[3 * i], saved[3 * i + 1]
                inp = outs[i - 1] if i > 0 else x
                k = inp.size(1)
                second_of_block, first_of_block = i > 0 and i % 2 == 0, i % 2 == 1
                if second_of_block:
                    block_grad = dy
                dz, dw, db, dg, dbe = new(n, w), new(w, k), new(w), new(w), new(w)
                check(L.snvc_fc_train_layer_backward_params(
                    _p(dy), _p(inp), _p(xhat), _p(gamma), _p(beta), _p(istd), _p(masks[i] if masks is not None else None), _p(dz),
                    _p(dg), _p(dbe), _p(dw), _p(db), n, k, w, keep_scale, leaky, stream), "snvc_fc_train_layer_backward_params")
                grads[4 * i:4 * i + 4] = [dw, db, dg, dbe]
                dx = new(n, k)
                check(L.snvc_fc_train_layer_backward_input(_p(dz), _p(weight), _p(block_grad if first_of_block else None), _p(dx),
                                                           n, k, w, stream), "snvc_fc_train_layer_backward_input")
                dy = dx
        return [dy] + grads

    # ------------------------------------------------------------------ the public calls
    def _run(self, x, representation):
        route = self._route(x)
        if route == "torch":
            y = self._torch_representation(x)
            return y if representation else self.w2(y)
        if route == "eval":
            return self._eval_forward(x, representation)
        n = x.size(0)
        if n == 1:      # what torch's batch_norm says for one value per channel
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([1, self.num_neurons])}")
        masks = self._draw_masks(n, x.device)
        if masks is not None and (masks.dtype != torch.uint8 or not masks.is_contiguous() or masks.device != x.device
                                  or tuple(masks.shape) != (1 + 2 * self.num_blocks, n, self.num_neurons)):
            raise RuntimeError("_draw_masks must give a contiguous uint8 [1 + 2 * num_blocks, N, num_neurons] tensor on the input's device")
        params = self._train_params()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _TrainFn.apply(self, masks, representation, x, *params)
        return self._train_forward(x, masks, representation, [p.detach() for p in params], keep=False)[0]

    def forward(self, x):
        return self._run(x, False)

    def get_representation(self, x):
        return self._run(x, True)


def get_fc_model():
    """The box head of ``VernierScale``: nine (x, z) pairs in, a five-number BEV box out (reference FCmodel.py:99-104)."""
    return FCModel(num_blocks=1, input_size=18, output_size=5, num_neurons=128)
