"""Drop-in for ``snvc.models.hrnet``: the HRNet feature backbone of ``VernierScale`` on the HIP kernels.

The public names, the module tree, the attribute names and therefore the state-dict keys, their order and their shapes
equal the reference's for any ``cfg.extra`` stage configuration and every ``head_type`` (hrnet.py:19-567), so a
reference checkpoint loads with ``strict=True``.  What changes is how ``forward`` executes for ``head_type == "default"``
on a float32 GPU tensor:

  reference (hrnet.py)                                   here
  ------------------------------------------------------ ------------------------------------------------------------
  stem, layer1, transitions, branch blocks: Conv2d,      one fused_conv2d launch per convolution: eval BatchNorm
    BatchNorm2d, ReLU, residual add      :25-110,420-445   folded, ReLU and the block's residual add in the epilogue
  fusion of output branch i              :184-258        down paths j < i: 3x3 stride-2 chains, the last layer adds
    (Upsample'd terms materialised, pairwise adds, ReLU)    the running partial sum in its epilogue; up paths j > i:
                                                           the 1x1 layer + BN at its own resolution; then ONE launch
                                                           of snvc_hrnet_fuse_forward sums x_i and the low-resolution
                                                           terms (nearest upsampling on the fly) and applies the ReLU

Under autograd, or with train-mode BatchNorm, the convolutions go through ``_Conv2dNormActFn`` as the 2D neck's do and
the fusion sum through ``_FuseSumFn``, whose backward is snvc_hrnet_fuse_backward, so ``VernierScale`` trains through
its backbone natively.  The other head types and anything that is not a float32 tensor with BatchNorm2d everywhere
run the same modules' torch forward.  Every decision is counted in ``submodule._ROUTES`` as "hrnet_hip" or
"hrnet_torch"; ``HRNET_HIP[0] = False`` forces the torch route (the same-module baseline of the tests and of
tools/bench_hrnet.py).  There is no CPU path: a CPU input raises.

The input must be a multiple of 32 in both extents, as in the reference, whose ``y + ...`` fails otherwise; here the
fusion kernel rejects the mismatched extent.
"""
import logging
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hrnet
from .submodule import _ROUTES, _norms2d, fused_conv2d
from .submodule import BasicBlock2d as BasicBlock
from .submodule import basicdownsample  # noqa: F401  (public name of the reference module)

BN_MOMENTUM = 0.1
logger = logging.getLogger(__name__)

HRNET_HIP = [True]      # False: every HighResolutionNet / HighResolutionModule / Bottleneck takes the modules' torch forward


def conv3x3(in_planes, out_planes, stride=1):
    """hrnet.py:19-22"""
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


def _bn(c):
    return nn.BatchNorm2d(c, momentum=BN_MOMENTUM)


class Bottleneck(nn.Module):
    """hrnet.py:72-110"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        wide = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = _bn(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = _bn(planes)
        self.conv3 = nn.Conv2d(planes, wide, kernel_size=1, bias=False)
        self.bn3 = _bn(wide)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        return _block(self, x, _hip_ok(x, self))


blocks_dict = {"basic": BasicBlock, "bottleneck": Bottleneck}


# ------------------------------------------------------------------------------------------
# the two routes, block by block
# ------------------------------------------------------------------------------------------
def _hip_ok(x: torch.Tensor, module: nn.Module, default_head: bool = True) -> bool:
    """The HIP route: a float32 GPU tensor, BatchNorm2d as every norm, the "default" head and ``HRNET_HIP[0]``."""
    if not x.is_cuda:
        raise RuntimeError("HRNet input must be a GPU tensor: Not implemented on the CPU")
    ok = (HRNET_HIP[0] and default_head and x.dtype == torch.float32
          and all(isinstance(n, nn.BatchNorm2d) for n in _norms2d(module)))
    _ROUTES["hrnet_hip" if ok else "hrnet_torch"] += 1
    return ok


def _block(b, x, hip):
    """BasicBlock (hrnet.py:37-54) or Bottleneck (:88-110): relu(bn_last(conv_last(...)) + residual)."""
    convs = [(b.conv1, b.bn1), (b.conv2, b.bn2)] + ([(b.conv3, b.bn3)] if isinstance(b, Bottleneck) else [])
    if hip:
        residual = x if b.downsample is None else fused_conv2d(b.downsample[0], b.downsample[1], x)
        out = x
        for conv, bn in convs[:-1]:
            out = fused_conv2d(conv, bn, out, relu=True)
        return fused_conv2d(convs[-1][0], convs[-1][1], out, relu=True, residual=residual)      # residual in the epilogue
    out = x
    for conv, bn in convs[:-1]:
        out = F.relu(bn(conv(out)))
    out = convs[-1][1](convs[-1][0](out))
    residual = x if b.downsample is None else b.downsample(x)
    return F.relu(out + residual)


def _blocks(seq, x, hip):
    for b in seq:
        x = _block(b, x, hip)
    return x


def _cbr(layer, x, hip):
    """Sequential(Conv2d, BatchNorm2d[, ReLU]) of the transitions and down paths."""
    if hip:
        return fused_conv2d(layer[0], layer[1], x, relu=len(layer) > 2)
    return layer(x)


def _chain(seq, x, hip):
    for layer in seq:
        x = _cbr(layer, x, hip)
    return x


def _transition(layer, x, hip):
    """A transition: one Sequential(Conv2d, BatchNorm2d, ReLU), or a chain of them for a new branch."""
    return _chain(layer, x, hip) if isinstance(layer[0], nn.Sequential) else _cbr(layer, x, hip)


class _FuseSumFn(torch.autograd.Function):
    """relu(t0 + up(t1) + ...) with the HIP backward: one pass over gy and out gives the masked gradient (shared by every
    factor-1 term) and the block sums of every up-sampled term."""

    @staticmethod
    def forward(ctx, factors, *terms):
        out = _hrnet.fuse_forward(list(terms), factors, relu=True)
        ctx.factors = factors
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        out, = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:]
        g = _hrnet.fuse_backward(gy.contiguous(), out, [f for f, n in zip(ctx.factors, needs) if n])
        return (None,) + tuple(g[f] if n else None for f, n in zip(ctx.factors, needs))


def _fuse_sum(terms, factors, in_place):
    """One launch of the fusion kernel; through ``_FuseSumFn`` when a term wants a gradient, in place into term 0 when
    ``in_place`` (term 0 is then a temporary of the caller's)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in terms):
        return _FuseSumFn.apply(tuple(factors), *terms)
    return _hrnet.fuse_forward(terms, factors, relu=True, out=terms[0] if in_place else None)


def _module_hip(m, xs):
    """HighResolutionModule.forward (hrnet.py:235-252) on the HIP route."""
    xs = [_blocks(m.branches[i], xs[i], True) for i in range(m.num_branches)]
    if m.num_branches == 1:
        return xs
    outs = []
    for i in range(len(m.fuse_layers)):
        part = None                                         # sum of the down paths j < i, in order j = 0, 1, ...
        for j in range(i):
            path = m.fuse_layers[i][j]
            t = _chain(path[:-1], xs[j], True)
            part = fused_conv2d(path[-1][0], path[-1][1], t, residual=part)         # bn(conv(t)) + part, no activation
        terms = ([part] if part is not None else []) + [xs[i]]
        factors = [1] * len(terms)
        for j in range(i + 1, m.num_branches):
            up = m.fuse_layers[i][j]
            terms.append(fused_conv2d(up[0], up[1], xs[j]))                          # 1x1 + BN at its own resolution
            factors.append(2 ** (j - i))
        outs.append(_fuse_sum(terms, factors, in_place=part is not None))
    return outs


def _module_torch(m, xs):
    """HighResolutionModule.forward (hrnet.py:235-252) with the modules' own torch forward."""
    xs = [_blocks(m.branches[i], xs[i], False) for i in range(m.num_branches)]
    if m.num_branches == 1:
        return xs
    outs = []
    for i in range(len(m.fuse_layers)):
        y = xs[0] if i == 0 else m.fuse_layers[i][0](xs[0])
        for j in range(1, m.num_branches):
            y = y + (xs[j] if i == j else m.fuse_layers[i][j](xs[j]))
        outs.append(m.relu(y))
    return outs


class HighResolutionModule(nn.Module):
    """hrnet.py:113-258"""

    def __init__(self, num_branches, blocks, num_blocks, num_inchannels, num_channels, fuse_method, multi_scale_output=True):
        super().__init__()
        for name, seq in (("NUM_BLOCKS", num_blocks), ("NUM_CHANNELS", num_channels), ("NUM_INCHANNELS", num_inchannels)):
            if len(seq) != num_branches:
                msg = f"NUM_BRANCHES({num_branches}) <> {name}({len(seq)})"
                logger.error(msg)
                raise ValueError(msg)
        # the list is the caller's and is updated in place with each branch's output width, as in the reference (:147-150)
        self.num_inchannels = num_inchannels
        self.fuse_method = fuse_method
        self.num_branches = num_branches
        self.multi_scale_output = multi_scale_output
        self.branches = self._make_branches(num_branches, blocks, num_blocks, num_channels)
        self.fuse_layers = self._make_fuse_layers()
        self.relu = nn.ReLU(False)

    def _make_one_branch(self, branch_index, block, num_blocks, num_channels, stride=1):
        cin, width = self.num_inchannels[branch_index], num_channels[branch_index] * block.expansion
        downsample = None
        if stride != 1 or cin != width:
            downsample = nn.Sequential(nn.Conv2d(cin, width, kernel_size=1, stride=stride, bias=False), _bn(width))
        layers = [block(cin, num_channels[branch_index], stride, downsample)]
        self.num_inchannels[branch_index] = width
        layers += [block(width, num_channels[branch_index]) for _ in range(1, num_blocks[branch_index])]
        return nn.Sequential(*layers)

    def _make_branches(self, num_branches, block, num_blocks, num_channels):
        return nn.ModuleList([self._make_one_branch(i, block, num_blocks, num_channels) for i in range(num_branches)])

    def _make_fuse_layers(self):
        if self.num_branches == 1:
            return None
        c = self.num_inchannels
        rows = []
        for i in range(self.num_branches if self.multi_scale_output else 1):
            row = []
            for j in range(self.num_branches):
                if j > i:           # 1x1 to branch i's width, then nearest upsampling
                    row.append(nn.Sequential(nn.Conv2d(c[j], c[i], 1, 1, 0, bias=False), _bn(c[i]),
                                             nn.Upsample(scale_factor=2 ** (j - i), mode="nearest")))
                elif j == i:
                    row.append(None)
                else:               # i - j stride-2 3x3 layers; only the last changes the width, and has no ReLU
                    steps = []
                    for k in range(i - j):
                        if k == i - j - 1:
                            steps.append(nn.Sequential(nn.Conv2d(c[j], c[i], 3, 2, 1, bias=False), _bn(c[i])))
                        else:
                            steps.append(nn.Sequential(nn.Conv2d(c[j], c[j], 3, 2, 1, bias=False), _bn(c[j]), nn.ReLU(False)))
                    row.append(nn.Sequential(*steps))
            rows.append(nn.ModuleList(row))
        return nn.ModuleList(rows)

    def get_num_inchannels(self):
        return self.num_inchannels

    def forward(self, x):
        return (_module_hip if _hip_ok(x[0], self) else _module_torch)(self, list(x))


class HighResolutionNet(nn.Module):
    """hrnet.py:267-567"""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        if kwargs.get("head_type") != "heatmap_regression":
            self.conv1 = nn.Conv2d(3, 64, kernel_size=3, stride=2, padding=1, bias=False)
            self.bn1 = _bn(64)
            self.conv2 = nn.Conv2d(64, 64, kernel_size=3, stride=2, padding=1, bias=False)
            self.bn2 = _bn(64)
            self.relu = nn.ReLU(inplace=True)

        self.stage1_cfg = cfg.extra.stage1
        block = blocks_dict[self.stage1_cfg.block]
        width1 = self.stage1_cfg.num_channels[0]
        self.layer1 = self._make_layer(block, 64, width1, self.stage1_cfg.num_blocks[0])
        pre = [block.expansion * width1]
        for s in (2, 3, 4):
            stage_cfg = getattr(cfg.extra, f"stage{s}")
            setattr(self, f"stage{s}_cfg", stage_cfg)
            exp = blocks_dict[stage_cfg.block].expansion
            widths = [w * exp for w in stage_cfg.num_channels]
            setattr(self, f"transition{s - 1}", self._make_transition_layer(pre, widths))
            stage, pre = self._make_stage(stage_cfg, widths, multi_scale_output=True)
            setattr(self, f"stage{s}", stage)

        self.head_type = kwargs["head_type"] if "head_type" in kwargs else cfg.head_type
        if self.head_type == "default":
            pass
        elif self.head_type == "classification":
            self.incre_modules, self.downsamp_modules, self.final_layer = self._make_head(pre)
            self.classifier = nn.Linear(2048, 1000)
        elif self.head_type == "heatmap_regression":
            self.upsamp_fact = 2
            self.final_layer_hm = nn.Sequential(nn.Conv2d(pre[0], 9 * self.upsamp_fact ** 2, kernel_size=1, stride=1, padding=0),
                                                nn.PixelShuffle(self.upsamp_fact))
        else:
            raise NotImplementedError

    def _make_head(self, pre_stage_channels):
        """hrnet.py:361-408"""
        head_channels = [32, 64, 128, 256]
        exp = Bottleneck.expansion
        incre = nn.ModuleList([self._make_layer(Bottleneck, c, head_channels[i], 1, stride=1) for i, c in enumerate(pre_stage_channels)])
        down = nn.ModuleList([
            nn.Sequential(nn.Conv2d(in_channels=head_channels[i] * exp, out_channels=head_channels[i + 1] * exp, kernel_size=3, stride=2,
                                    padding=1),
                          _bn(head_channels[i + 1] * exp), nn.ReLU(inplace=True))
            for i in range(len(pre_stage_channels) - 1)])
        final = nn.Sequential(nn.Conv2d(in_channels=head_channels[3] * exp, out_channels=2048, kernel_size=1, stride=1, padding=0),
                              _bn(2048), nn.ReLU(inplace=True))
        return incre, down, final

    def _make_transition_layer(self, num_channels_pre_layer, num_channels_cur_layer):
        """hrnet.py:410-443: a 3x3 layer where an existing branch changes width, a chain of stride-2 layers for a new one."""
        n_pre = len(num_channels_pre_layer)
        layers = []
        for i, cur in enumerate(num_channels_cur_layer):
            if i < n_pre:
                prev = num_channels_pre_layer[i]
                layers.append(None if cur == prev else
                              nn.Sequential(nn.Conv2d(prev, cur, 3, 1, 1, bias=False), _bn(cur), nn.ReLU(inplace=True)))
                continue
            cin = num_channels_pre_layer[-1]
            steps = []
            for j in range(i + 1 - n_pre):
                cout = cur if j == i - n_pre else cin
                steps.append(nn.Sequential(nn.Conv2d(cin, cout, 3, 2, 1, bias=False), _bn(cout), nn.ReLU(inplace=True)))
            layers.append(nn.Sequential(*steps))
        return nn.ModuleList(layers)

    def _make_layer(self, block, inplanes, planes, blocks, stride=1):
        """hrnet.py:445-460"""
        width = planes * block.expansion
        downsample = None
        if stride != 1 or inplanes != width:
            downsample = nn.Sequential(nn.Conv2d(inplanes, width, kernel_size=1, stride=stride, bias=False), _bn(width))
        return nn.Sequential(block(inplanes, planes, stride, downsample), *[block(width, planes) for _ in range(1, blocks)])

    def _make_stage(self, layer_config, num_inchannels, multi_scale_output=True):
        """hrnet.py:462-489"""
        block = blocks_dict[layer_config.block]
        modules = []
        for i in range(layer_config.num_modules):
            multi = multi_scale_output or i != layer_config.num_modules - 1
            modules.append(HighResolutionModule(layer_config.num_branches, block, layer_config.num_blocks, num_inchannels,
                                                layer_config.num_channels, layer_config.fuse_method, multi))
            num_inchannels = modules[-1].get_num_inchannels()
        return nn.Sequential(*modules), num_inchannels

    # ------------------------------------------------------------------ forward
    def _stem(self, x, hip):
        if self.head_type == "heatmap_regression":
            return x
        if hip:
            x = fused_conv2d(self.conv1, self.bn1, x, relu=True)
            x = fused_conv2d(self.conv2, self.bn2, x, relu=True)
        else:
            x = self.relu(self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x))))))
        return _blocks(self.layer1, x, hip)

    def _stages(self, x, hip):
        run = _module_hip if hip else _module_torch
        ys = [x]
        for s in (2, 3, 4):
            n = getattr(self, f"stage{s}_cfg").num_branches
            trans = getattr(self, f"transition{s - 1}")
            # an unchanged branch passes through; a transition reads the last branch (hrnet.py:500-520)
            xs = [ys[i] if trans[i] is None else _transition(trans[i], ys[-1], hip) for i in range(n)]
            for m in getattr(self, f"stage{s}"):
                xs = run(m, xs)
            ys = xs
        return ys

    def forward(self, x):
        """hrnet.py:491-535"""
        hip = _hip_ok(x, self, default_head=self.head_type == "default")
        ys = self._stages(self._stem(x, hip), hip)
        if self.head_type == "default":
            return ys[0]
        if self.head_type == "heatmap_regression":
            return self.final_layer_hm(ys[0])
        y = _blocks(self.incre_modules[0], ys[0], False)
        for i in range(len(self.downsamp_modules)):
            y = _blocks(self.incre_modules[i + 1], ys[i + 1], False) + self.downsamp_modules[i](y)
        y = self.final_layer(y)
        if torch._C._get_tracing_state():
            y = y.flatten(start_dim=2).mean(dim=2)
        else:
            y = F.avg_pool2d(y, kernel_size=y.size()[2:]).view(y.size(0), -1)
        return self.classifier(y)

    def init_weights(self, pretrained=""):
        """hrnet.py:537-557: Kaiming-normal convolutions, unit BatchNorm; then every key of ``pretrained`` that this model has."""
        logger.info("=> init weights for 2D feature extraction from normal distribution")
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if os.path.isfile(pretrained):
            loaded = torch.load(pretrained)
            logger.info("=> loading pretrained model %s", pretrained)
            state = self.state_dict()
            matched = {k: v for k, v in loaded.items() if k in state}
            for k in matched:
                print(f"=> loading {k} pretrained model {pretrained}")
                logger.info("=> loading %s pretrained model %s", k, pretrained)
            state.update(matched)
            self.load_state_dict(state)

    def modify_input_channel(self, num_channels):
        """hrnet.py:559-569: a wider first layer whose first three input channels keep the old weights.  The new layer is
        registered anew, so its key moves to the end of the state dict as in the reference."""
        if num_channels == 3:
            return
        wider = nn.Conv2d(num_channels, 64, kernel_size=3, stride=2, padding=1, bias=False)
        with torch.no_grad():
            wider.weight[:, :3, :, :] = self.conv1.weight.clone()
        del self.conv1
        self.conv1 = wider


def get_model(cfg, is_train, **kwargs):
    """hrnet.py:571-579"""
    model = HighResolutionNet(cfg, **kwargs)
    if is_train and cfg.init_weights:
        model.init_weights(cfg.pre_trained_path)
    if getattr(cfg, "add_xy", False):
        model.modify_input_channel(5)
    return model
