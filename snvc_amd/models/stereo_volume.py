"""Global scene stack: plane-sweep cost volume -> 3D convs -> hourglass -> classifier.

The public reference does not ship its global model (``snvc/models/__init__.py:1-2`` has the
``StereoNet`` imports commented out); what it does ship is the op (``build_cost_volume``), the
blocks (``convbn_3d``, ``hourglass``) and the composition pattern of VernierScale's '3D' branch
(vernier.py:128-142 constructor, :366-371 forward -- itself dead code upstream: it defines
``hg_conv`` but calls ``hg_conv3d``).  ``GlobalStack`` is that pattern on a concat cost volume
(BASELINE.json configs[0..1]):

    volume = build_cost_volume(left, right, shift, ds)          [N, 2C, D, H, W]
    v = relu(bn(conv3(volume)))   2C -> C                        conv1
    v = relu(bn(conv3(v)))        C  -> C                        conv2
    v = v + hourglass(v)[0]                                      hg_conv3d
    cost = conv1x1x1(v)           C  -> 1                        classifier
"""
import dataclasses
import itertools
import warnings
import weakref

import torch
import torch.nn as nn

from ..extension.build_cost_volume import _BuildCostVolume, build_cost_volume  # noqa: F401  (re-exported)
from .. import ops
from .._derived import derived, fresh, stamp
from .submodule import (_ROUTES, SCRATCH_ATTRS, WORKSPACE_ATTRS, X3_GROUP_NORM, ConvBNReLU3d, HipConv3d, SplitModePolicy, SplitOverflow,
                        SplitT, _FactoredFirstConvFn, _ShearedFirstConvBNFn, _ShearedFirstConvFn, _folded_bn,
                        _is_channel_head as _is_head_conv, _Plan, convbn_3d, folded_head_weights, hourglass, overflow_guard, plan_for,
                        sheared_geometry, sheared_kernels, x3_exponent, x3_norm_bound, EPI_RELU, SHEAR_CLASS_KDS)

_PREP_EPOCH = itertools.count(1)      # stamps of the per-model first-layer prep buffers (see _factored_pair_steps)
_X3_KEY = {ops.Conv3dLayer: "", ops.Conv2dLayerX3: "_x3"}      # plan-dict key suffix of a depth-1 layer kind (GlobalStack._layers)
POOLED_PREP_CALLS = 0                 # pooled first-layer preps queued (GlobalStack.pooled_prep): counted here, _ROUTES' key set is pinned
_ASK = object()                       # _conv2_tail: the caller has not resolved the split-mode state


@dataclasses.dataclass
class _Prep:
    """What the first layer's small 2D launches of ONE step share (GlobalStack._left_planes, _sheared_inputs, _commuted_inputs) and what
    its expand pass needs of them."""
    plans: dict                       # _factored_plans(conv1, c): the layers of every weight fold
    c: int                            # feature channels: `weight` is conv1's [Cout, 2 c, 3, 3, 3], left half first
    weight: torch.Tensor
    st: dict = None                   # this step's split-mode state (_x3_select), None: fp32 arithmetic
    scale: torch.Tensor = None        # the folded eval BatchNorm (None: a GroupNorm layer, statistics per call)
    bias: torch.Tensor = None
    split_prep: bool = False          # the 2D layers in split mode too, results in `prep_ws` (False: fp32 MFMA, results from the allocator)
    fuse: bool = False                # ... and channel-interleaved copies (`p_il`, G | G') for conv2's fused first layer
    prep_ws: dict = None
    planes: torch.Tensor = None       # [N, c, 3, H, W], filled by _left_planes
    p_il: torch.Tensor = None


def _factored_plans(conv: nn.Module, c: int) -> dict:
    """The factored first layer's packed right half ("right"), its folded-BatchNorm plan ("plan") and what the routes add to the
    dict lazily: all of it rebuilt when the weight changes."""
    plans = conv.__dict__.get("_snvc_factored")
    if plans is None or not fresh(plans["stamp"], (conv.weight,)):
        w = conv.weight
        plans = conv.__dict__["_snvc_factored"] = {"stamp": stamp((w,)), "plan": _Plan(),
                                                   "right": ops.Conv3dLayer(w.detach()[:, c:].contiguous(), 3, 1, 1, 1, False)}
    return plans


def _mark(timing, name, which):
    """Record the start (0) / end (1) event of bracket ``name`` on the current stream, if the caller asked for that bracket."""
    if timing is not None and name in timing:
        timing[name][which].record()


def _run(gen):
    """A generator run to its end: its return value."""
    try:
        while True:
            next(gen)
    except StopIteration as done:
        return done.value


class GlobalStack(SplitModePolicy, nn.Module):
    def __init__(self, c=32, gn=False):
        super().__init__()
        self.conv1 = ConvBNReLU3d(convbn_3d(2 * c, c, 3, 1, 1, gn=gn), nn.ReLU(inplace=True))
        self.conv2 = ConvBNReLU3d(convbn_3d(c, c, 3, 1, 1, gn=gn), nn.ReLU(inplace=True))
        self.hg_conv3d = hourglass(c, gn=gn)
        self.classifier = HipConv3d(c, 1, kernel_size=1, padding=0, stride=1, bias=False)
        for m in self.modules():  # same init as VernierScale (vernier.py:38-46)
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm3d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _buffer(self, name, shape, device, dtype=torch.float32):
        """Inference workspace: the three full-resolution intermediates (warped half-volume, conv1 / conv2 outputs,
        0.74 GB each at cfg2) are kept across calls instead of going through the caching allocator every step -- with
        GB-sized blocks that are split and re-merged, a steady-state step can land on a fresh hipMalloc (tens of ms).
        They never escape ``forward`` / ``forward_pair`` (the result is the head's own small tensor).
        One buffer per (name, device): replicas on different devices keep their own.  Single-stream: the buffers
        are not tracked by the caching allocator's stream bookkeeping, so calls on two streams of one device would
        alias them.  ``release_workspace()`` / ``invalidate_plans(model)`` / ``train()`` give the memory back."""
        ws = self.__dict__.setdefault("_snvc_ws", {})
        key = (name, tuple(shape), device)
        buf = ws.get(key)
        if buf is None:
            for k in [k for k in ws if k[0] == name and k[2] == device]:
                del ws[k]
            buf = ws[key] = torch.empty(shape, dtype=dtype, device=device)
        return buf

    # The two first-layer buffers.  They are the only places that say where the call's first-layer result is (last_first_layer()).
    def _v1(self, shape, device):
        """The fp32 first-layer result [N,C,D,H,W]."""
        self.__dict__["_snvc_last_v1"] = "v1"
        return self._buffer("v1", shape, device)

    def _v1s(self, shape, device, last="v1s", lazy=None):
        """The split pair [N,2,C/8,D,H,W,8] of a first-layer result of fp32 ``shape``.  ``last="v1"``: the pair is a layout pass over the
        fp32 result, which is in the workspace too.  ``lazy`` (the fused route, which never stores the pair): nothing is handed out;
        ``lazy(pair buffer)`` fills it if somebody asks for the result."""
        def pair():
            return self._buffer("v1s", (shape[0], 2, shape[1] // 8) + tuple(shape[2:]) + (8,), device, torch.float16)
        if lazy is not None:
            self.__dict__.setdefault("_snvc_ws", {})[("v1s_lazy", (), None)] = lambda: lazy(pair())
            self.__dict__["_snvc_last_v1"] = "v1s_lazy"
            return None
        self.__dict__["_snvc_last_v1"] = last
        return pair()

    def last_first_layer(self) -> torch.Tensor:
        """The first layer's result of the most recent inference call as a float32 [N,C,D,H,W] tensor (a copy when the call ran
        in split mode and the workspace holds the (hi, lo) pair) -- for tests and debugging."""
        ws = self.__dict__.get("_snvc_ws", {})
        which = self.__dict__.get("_snvc_last_v1", "v1")
        if which == "v1s_lazy":      # the fused route never stored it: the expand pass on the operands the call left in the prep workspace
            return ops.from_split(ws[("v1s_lazy", (), None)](), self.__dict__["_snvc_x3"]["exp"]["v1"])
        for k, v in ws.items():
            if k[0] == which == "v1s":
                st = self.__dict__.get("_snvc_x3")      # None: a GroupNorm stack, whose sheared first layer takes the exponent from the norm's bound
                return ops.from_split(v, st["exp"]["v1"] if st is not None else
                                      x3_exponent(x3_norm_bound(self.conv1[0][1], plan_for(self.conv1[0][0], "_x3", v.device))))
            if k[0] == which:
                return v
        raise RuntimeError("no first-layer result in the workspace")

    def release_workspace(self):
        """Drop the persistent inference workspace (2.2 GB at cfg2)."""
        for name in WORKSPACE_ATTRS:
            self.__dict__.pop(name, None)

    def train(self, mode: bool = True):
        if mode:
            self.release_workspace()
        return super().train(mode)

    def __getstate__(self):          # copy.deepcopy / torch.save(model): workspace, packed split-mode layers, overflow flag are scratch
        state = self.__dict__.copy()
        for name in SCRATCH_ATTRS:
            state.pop(name, None)
        return state

    # ------------------------------------------------------------------------------------------ split mode ("f16x3", r4)
    # Inference with frozen statistics: conv2 and the hourglass's five MFMA layers run on the split-mode kernels
    # (csrc/conv3d_f16.hip, F16Cfg::PL): the SAME fp32 layers -- values travel as (hi, lo) pairs of halves (22 bits), a product
    # is three v_mfma_f32_32x32x16_f16 with fp32 accumulation, measured 5e-7 of the range against float64 where the fp32
    # Winograd kernels measure 2e-6 -- on a matrix pipe 16 times faster than the fp32 one.  ``arithmetic``: "auto" (default:
    # split mode when the stack qualifies), "fp32" (the fp32-MFMA kernels everywhere), "x3" (split mode or an error).
    # What happens when a value leaves a split tensor's range (``overflow_check``, ``check_overflow()``, ``reset_split_mode()``):
    # split_mode.SplitModePolicy.
    arithmetic = "auto"
    # the first layer's 0.74 GB split pair written with non-temporal stores (SNVC_EPI_STREAM_OUT): the expand pass alone gains 9 % (182 ->
    # 165 us back to back) but the step LOSES 0.013 ms (tools/ab_step.py, profiles/r5/ab_step_v5.txt): conv2 reads the pair right
    # behind it.  Off.
    stream_out = False
    # split mode, sheared route, q = 1 | 2: conv2's launch forms the first layer's result itself from G | G' and the left planes
    # (csrc/conv3d_f16.hip, conv3d_x3q_kernel<EPI, 1>): the expand pass, its 0.74 GB pair and conv2's reads of it are gone.  Same bits.
    # False: the expand pass writes the pair, conv2 reads it (every other route does that anyway).
    fused_first = True
    # the fused first layer's wedge (include/snvc_dedup.h): left of the image's first column the volume does not depend on the plane,
    # so conv2's tiles that lie wholly there (8.3 % at cfg2) are computed once per (row, column) and copied.  Same bits.  False: every
    # tile is computed.
    dedup_wedge = True
    # the duplicates are not copied either (include/snvc_alias.h): their rows of v2s and of the side head stay unwritten, and the one
    # reader of each -- the hourglass's first stride-2 layer, the tail's gather -- reads the representative's row in their place.  Same
    # bits.  Taken only with dedup_wedge and fused_first on the fused-tail route, where that stride-2 layer runs on its persistent
    # 16x16x32 form and the shape has duplicates; anything else is the copy route.  False: the copy route.
    alias_wedge = True
    # on the alias route the hourglass's first stride-2 layer does not compute its own duplicate tiles either (include/snvc_hgdedup.h:
    # 144 of its 2 880 jobs at cfg2), and hg conv2 -- the one reader of its result -- reads the representative's rows.  Same bits.  Taken
    # only where the shape has such tiles and both layers run on their 16x16x32 forms; anything else is the alias route's own calls.
    dedup_hourglass = True
    # the fused first layer's 2D prep -- both features' scales, the three split pairs, G / G' / the left planes -- is queued as three pooled
    # launches instead of eight (include/snvc_prep.h) wherever the sheared inputs are queued anyway (spacing known, or guessed for this
    # shape).  Same bits.  False, or any other case: the two calls' own launches.
    pooled_prep = True
    # ... with the left planes' layer packed class-major (il_mode 2): the interleaved copy leaves as two 16-byte stores per lane
    # instead of eight 4-byte ones.  Same bits.
    planes_class_major = True
    split_prep = True    # split mode: the sheared first layer's depth-1 3 x 7 layers (G, G') on the half pipe too (False: fp32 MFMA, as r4)
    fused_tail = True    # split mode: conv5's epilogue contracts its result with the folded one-channel tail (False: r4's two launches)

    def _x3_state(self, device):
        """Packed split-mode layers, folded affines and per-tensor exponents of conv2 + the hourglass, or None when the stack
        does not qualify (channels, norm kind, train mode).  Cached on the parameters' versions."""
        hg = self.hg_conv3d
        seqs = {"conv2": self.conv2[0], "h1": hg.conv1[0], "h2": hg.conv2, "h3": hg.conv3[0], "h4": hg.conv4[0], "h5": hg.conv5}
        c = self.conv2[0][0].out_channels
        if c != 32 or self.conv2[0][0].in_channels != 32 or not _is_head_conv(self.classifier, c):
            return None
        norms = [self.conv1[0][1]] + [sq[1] for sq in seqs.values()]
        for nm in norms:
            if not isinstance(nm, nn.BatchNorm3d) or nm.training or nm.running_mean is None:
                return None
        tensors = [t for sq in list(seqs.values()) + [hg.conv6] for t in (sq[0].weight, sq[1].weight, sq[1].bias, sq[1].running_mean, sq[1].running_var)]
        tensors.append(self.classifier.weight)
        tensors += [self.conv1[0][1].weight, self.conv1[0][1].bias, self.conv1[0][1].running_mean, self.conv1[0][1].running_var]
        st = self.__dict__.get("_snvc_x3")
        if st is not None and fresh(st["stamp"], tensors, (device,)):
            return st
        e = {k: x3_exponent(x3_norm_bound(sq[1], plan_for(sq[0], "_x3", device))) for k, sq in [("v1", self.conv1[0])] + list(seqs.items())}
        st = {"stamp": stamp(tensors, (device,)), "exp": e, "layers": {}, "affine": {}}
        geo = {"conv2": (1, False), "h1": (2, False), "h2": (1, False), "h3": (2, False), "h4": (1, False), "h5": (2, True)}
        for k, sq in seqs.items():
            w = sq[0].weight.detach().to(device)
            st["layers"][k] = ops.Conv3dLayerX3(w, 3, geo[k][0], 1, 1, geo[k][1])
            st["affine"][k] = _folded_bn(sq[1], plan_for(sq[0], "", device))
        # `post` = relu(bn(conv5(o)) + pre) exists only inside conv5's epilogue (below); its exponent comes from a HARD bound, not from
        # the statistical one: |conv5(o)| <= (sum of |w| over a parity class's taps and all input channels) * max|o|, and o / pre cannot
        # exceed what their own (checked) exponents allow.  conv5 then cannot clamp once the layers before it have not, so the overflow
        # flag is final BEHIND hg conv4 and the host's look at it overlaps conv5 + the gather (0.17 ms of GPU work) instead of
        # leaving the GPU empty for the next call's first launches (r5: 0.08 ms per step).  The price: ~3 bits of exponent headroom
        # out of half's 30 -- nothing, for activations of ordinary magnitude.
        w5 = hg.conv5[0].weight.detach().double().abs()                       # [Cin, Cout, 3, 3, 3]
        sets = ([1], [0, 2])
        l1 = None
        for pd in range(2):
            for ph in range(2):
                for pw in range(2):
                    t = w5[:, :, sets[pd]][:, :, :, sets[ph]][:, :, :, :, sets[pw]].sum(dim=(0, 2, 3, 4))
                    l1 = t if l1 is None else torch.maximum(l1, t)
        sc5, bi5 = st["affine"]["h5"]
        hard = float(((sc5.double().abs() * l1.to(sc5.device) * (65504.0 / 2.0 ** st["exp"]["h4"]) + bi5.double().abs()).max()
                      + 65504.0 / 2.0 ** st["exp"]["h2"]).item())
        st["exp"]["post"] = min(x3_exponent(hard), st["exp"]["h2"])
        # the folded tail classifier(bn(conv6(post)) + v): a transposed layer to one channel whose per-voxel tap contraction is part
        # of conv5's epilogue (snvc_f16x3_deconv3d_tail_forward); `post` is never stored
        st["tail"] = st["tail_bias"] = None
        if isinstance(hg.conv6[1], nn.BatchNorm3d) and not hg.conv6[1].training and hg.conv6[0].in_channels % 32 == 0:
            wf, fb = folded_head_weights(hg.conv6[0], hg.conv6[1], self.classifier)
            st["tail"] = ops.TailWeightsX3(wf.float().to(device))
            st["tail_bias"] = fb.float().reshape(1).to(device)
        st["guard"] = overflow_guard(self, device)      # survives rebuilds of this state: a pending flag is never dropped
        st["flag"] = st["guard"].flag
        self.__dict__["_snvc_x3"] = st
        return st

    @staticmethod
    def _x3_v1_affine(st, scale, bias):
        """The first layer's folded BatchNorm with the exponent of the split first-layer tensor folded in (exact: a power of two)."""
        e1 = st["exp"]["v1"]
        return derived(st, "v1_affine", (scale, bias), lambda: ((scale * 2.0 ** e1).contiguous(), (bias * 2.0 ** e1).contiguous()))

    def _x3_select(self, device, arithmetic=None):
        """The split-mode state if this call runs in split mode, else None."""
        mode = arithmetic or self.arithmetic
        if mode == "fp32" or torch.is_grad_enabled() or self.training or self.split_off:
            if mode == "x3":
                raise RuntimeError("arithmetic='x3' needs inference (no autograd, eval mode) and no earlier overflow")
            return None
        st = self._x3_state(device)
        if st is None:
            if mode == "x3":
                raise RuntimeError("arithmetic='x3': the stack does not qualify (32 channels, eval-mode BatchNorm3d everywhere)")
            return None
        return st if self.split_guard(device, mode) is not None else None      # None: overflow_check = "deferred", the previous call's flag

    def _tail_x3(self, st, v1s, timing=None, fused=None):
        """conv2 (+ side head) -> hourglass -> folded one-channel tail on a split-C8 first-layer result ``v1s`` (exponent
        st['exp']['v1']).  Full-resolution intermediates: v1s, v2s (0.74 GB each at cfg2, like their fp32 counterparts).
        ``fused`` (then ``v1s`` is None): ``(shape, device, kwargs)`` of ``Conv3dLayerX3.forward_fused_first`` -- conv2 forms v1s itself."""
        L, A, E, flag = st["layers"], st["affine"], st["exp"], st["flag"]
        if fused is not None:
            (n, _, d, h, w), dev = fused[0], fused[1]
        else:
            n, dev = v1s.size(0), v1s.device
            d, h, w = v1s.shape[3:6]
        hg = self.hg_conv3d
        _mark(timing, "conv2", 0)
        v2_out = self._buffer("v2s", (n, 2, 4, d, h, w, 8), dev, torch.float16)
        alias = None            # the descriptor of v2s / hv when their duplicate rows stay unwritten
        if fused is not None:
            if self._alias_route(st, n, (d, h, w), fused[2]):
                alias = ops.wedge_desc(d, w, fused[2]["q"], fused[2]["m0"], fused[2]["off"])
            v2s, hv = L["conv2"].forward_fused_first(n=n, in_sp=(d, h, w), x_exp=E["v1"], scale=A["conv2"][0], bias=A["conv2"][1], flags=EPI_RELU,
                                                     out_exp=E["conv2"], head=self.classifier.weight, overflow=flag, out=v2_out,
                                                     dedup=bool(self.dedup_wedge), alias=alias is not None, **fused[2])
            _ROUTES["fused_first_conv"] += 1
            _ROUTES["wedge_alias"] += alias is not None
        else:
            v2s, hv = L["conv2"](v1s, E["v1"], *A["conv2"], flags=EPI_RELU, out_exp=E["conv2"], head=self.classifier.weight, overflow=flag,
                                 out=v2_out)
        _mark(timing, "conv2", 1)
        _ROUTES["side_head"] += 1
        hg_dedup = alias is not None and self._hg_dedup_route(st, n, (d, h, w), alias)
        _ROUTES["hg_dedup"] += hg_dedup
        if hg_dedup:
            # its duplicate tiles are not computed (include/snvc_hgdedup.h); hg conv2, the result's one reader, aliases their rows
            o = L["h1"].forward_hg_dedup(v2s, alias, E["conv2"], *A["h1"], flags=EPI_RELU, out_exp=E["h1"], overflow=flag)
        elif alias is not None:
            o = L["h1"].forward_aliased(v2s, alias, E["conv2"], *A["h1"], flags=EPI_RELU, out_exp=E["h1"], overflow=flag)
        else:
            o = L["h1"](v2s, E["conv2"], *A["h1"], flags=EPI_RELU, out_exp=E["h1"], overflow=flag)              # 1/2 res, 2C channels
        if hg_dedup:
            pre = L["h2"].forward_hg_reader(o, alias, E["h1"], *A["h2"], flags=EPI_RELU, out_exp=E["h2"], overflow=flag)
        else:
            pre = L["h2"](o, E["h1"], *A["h2"], flags=EPI_RELU, out_exp=E["h2"], overflow=flag)                 # relu(bn(conv))   :153-156
        o = L["h3"](pre, E["h2"], *A["h3"], flags=EPI_RELU, out_exp=E["h3"], overflow=flag)                     # 1/4 res
        o = L["h4"](o, E["h3"], *A["h4"], flags=EPI_RELU, out_exp=E["h4"], overflow=flag)
        st["guard"].post()      # the last layer that can clamp (conv5's exponent is a hard bound, see _x3_state): the flag leaves for the host here
        if st["tail"] is not None and self.fused_tail:
            # post = relu(bn(deconv(o)) + pre) is formed and contracted with the folded tail's 27 taps inside conv5's launch (r5): 27
            # fp32 planes per parity class leave instead of 64 channels, and the last launch only sums them
            t = L["h5"].forward_tail(o, E["h4"], *A["h5"], st["tail"], residual=pre, res_exp=E["h2"], flags=EPI_RELU | ops.EPI_ADD_PRE,
                                     out_exp=E["post"], overflow=flag, out=self._buffer("tail_t", (n, 27, 8) + tuple(o.shape[3:6]), dev))
            cost = ops.deconv_tail_gather(t, st["tail_bias"], hv, res_alias=alias)            # deconv'(post) + b' + classifier(v2)
            _ROUTES["x3_fused_tail"] += 1
        else:
            # post = relu(bn(deconv(o)) + pre): the result leaves as fp32 NCDHW for the one-channel transposed tail (VALU kernel)
            post = L["h5"](o, E["h4"], *A["h5"], residual=pre, flags=EPI_RELU | ops.EPI_ADD_PRE, out_exp=E["h2"], to_f32=True)
            cost = hg.conv6.fused(post, residual=None, head=self.classifier, head_residual=hv)    # deconv'(post) + b' + classifier(v2)
        _ROUTES["x3_tail"] += 1
        if self.overflow_check == "call" and st["guard"].wait():
            # waited for while the transposed layer and the tail still run: this call's result is dropped and redone in fp32
            raise SplitOverflow()
        return cost

    def _alias_route(self, st, n, sp, src) -> bool:
        """True when this call's conv2 may leave the wedge's duplicate rows unwritten: both readers of v2s / hv then take the
        descriptor.  ``src``: the fused first layer's kwargs (q, m0, off)."""
        if not (self.alias_wedge and self.dedup_wedge and st["tail"] is not None and self.fused_tail):
            return False
        if not st["layers"]["h1"].aliased_form(n, sp):
            return False
        return ops.fused_first_wedge_dups(int(sp[0]), int(sp[2]), int(src["q"]), int(src["m0"]), int(src["off"])) > 0

    def _hg_dedup_route(self, st, n, sp, alias) -> bool:
        """True when, on the alias route, the hourglass's first stride-2 layer may leave ITS duplicate tiles out: the shape has some and
        both layers report the form -- hg conv1 the live walk, hg conv2 (the result's one reader) the aliased fill."""
        if not self.dedup_hourglass:
            return False
        L = st["layers"]
        return L["h1"].hg_dedup_form(n, sp, alias) and L["h2"].hg_reader_form(n, L["h1"].out_spatial(tuple(int(v) for v in sp)))

    def _tail(self, v, hv=None):
        """v + hourglass(v)[0] -> classifier.  The hourglass's last transposed layer has no activation
        (reference submodule.py:166), so at inference  classifier(bn(deconv(post)) + v) = deconv'(post) + b' +
        classifier(v)  with deconv' a transposed layer to ONE channel (fused_conv3d): the full-resolution C-channel
        tensor is never formed.  ``hv`` = classifier(v) when conv2's launch already produced it (side head)."""
        cost, _, _ = self.hg_conv3d(v, None, None, residual=v, head=self.classifier, head_residual=hv)
        return cost

    def _gn_qualifies(self, device, arithmetic=None):
        """The overflow guard if this call can run a GroupNorm stack in split mode (see _gn_tail_x3), else None."""
        mode = arithmetic or self.arithmetic
        norms = [m for m in self.modules() if isinstance(m, (nn.GroupNorm, nn.modules.batchnorm._BatchNorm))]
        if (not norms or not all(isinstance(m, nn.GroupNorm) for m in norms) or not X3_GROUP_NORM[0] or mode == "fp32"
                or torch.is_grad_enabled() or self.training or self.split_off or device.type != "cuda"
                or self.conv1[0][0].out_channels % 32 != 0):
            return None
        return self.split_guard(device, mode)

    def _gn_tail_x3(self, v1, timing=None, arithmetic=None):
        """A GroupNorm stack (``GlobalStack(gn=True)``) behind its fp32 first-layer result, in split mode (r5): nothing folds here
        (every norm needs its own conv result's statistics), so the layers run one by one through ``fused_conv3d_x3``'s GroupNorm
        form -- conv2, the hourglass, conv6 + cost0 -- and the 1x1x1 classifier on the fp32 kernel.  Returns None when the
        call does not qualify.  A flagged call raises SplitOverflow (``_checked`` redoes it in fp32)."""
        if isinstance(v1, SplitT):          # conv1 ran in split mode already (_forward_volume_unchecked): its guard is the caller's
            v1s, guard = v1, self.__dict__["_snvc_x3_guard"][v1.t.device]
        else:
            if not (v1.is_cuda and v1.dtype == torch.float32):
                return None
            guard = self._gn_qualifies(v1.device, arithmetic)
            if guard is None:
                return None
            norm1 = self.conv1[0][1]
            b1 = x3_norm_bound(norm1, plan_for(self.conv1[0][0], "_x3", v1.device))
            e1 = x3_exponent(b1)
            v1s = SplitT(ops.to_split(v1, e1, out=self._v1s(v1.shape, v1.device, last="v1")), e1, b1)
        _mark(timing, "conv2", 0)
        v2 = self.conv2.fused_x3(v1s, flag=guard.flag)
        _mark(timing, "conv2", 1)
        out, _, _ = self.hg_conv3d.forward_x3(v2, residual=v2, flag=guard.flag)
        guard.post()                      # nothing clamps behind this point
        cost = self.classifier(ops.from_split(out.t, out.exp))      # Conv3d(C, 1, k1): the fp32 kernel (the split one-channel form is k3)
        _ROUTES["x3_gn_tail"] += 1
        if self.overflow_check == "call" and guard.wait():
            raise SplitOverflow()
        return cost

    @staticmethod
    def _sheared_geometry4(m0: int, d: int, w: int):
        """sheared_geometry for four phases (index 4 w - d - m0): the kernel's taps reach 5 elements either side, so Rq sits 8 elements
        into its padded grid and the last column's window carries 5 elements of context."""
        off = 8
        wu = (off + 4 * (w - 1) + 1 + 5 + 5 + 3) // 4 * 4
        u_lo = 4 * (w - 1) - (d - 1) - m0 - 5
        return off, wu, 8 - u_lo, (d + 10 + 8 + 3) // 4 * 4

    @staticmethod
    def _sheared_layer4(plans, wr):
        """Four phases: G[u] = sum over (kd, kh, kw) of w[kd, kh, kw] Rq[row + kh - 1][u + 4 kw - kd] is a 3 x 11 kernel with nine non-zero
        columns = three 3 x 3 layers P_kw[u] = sum_{kd, kh} w[kd, kh, kw] Rq[row + kh - 1][u - kd] added 4 elements apart:
        G[u] = P_-1[u - 4] + P_0[u] + P_+1[u + 4], and G' (the last column: no kw = +1 taps) = P_-1[u - 4] + P_0[u].  One depth-1 3 x 3
        layer with 3 (kw) x 3 (depth class) x Cout output channels, folded in fp64 like sheared_kernels."""
        def fold():
            w = wr.detach().double()                                        # [Cout, C, kd, kh, kw]
            cout, c = w.shape[0], w.shape[1]
            k = torch.zeros((3, 3, cout, c, 3, 3), dtype=torch.float64, device=w.device)      # [kw][cls][co][c][kh][1 - kd]
            for cls, kds in enumerate(SHEAR_CLASS_KDS):
                for kd in kds:
                    for kw in (-1, 0, 1):
                        k[kw + 1, cls, :, :, :, 1 - kd] += w[:, :, kd + 1, :, kw + 1]
            return [k.reshape(9 * cout, c, 3, 3)]
        return GlobalStack._layers(plans, "sheared4", ops.Conv3dLayer, fold)[0]

    def _sheared4_inputs(self, plans, wr, rq_src, q_up, m0, d, w):
        """(g, gcol, off, off_col) of the four-phase sheared layer: ``rq_src`` upsampled by ``q_up`` (1 or 2) is Rq."""
        lay = self._sheared_layer4(plans, wr)
        off, wu, off_col, wu_col = self._sheared_geometry4(m0, d, w)
        out = []
        for width, o_, last in ((wu, off, False), (wu_col, off_col, True)):
            p = lay(ops.sheared_upsample(rq_src, q_up, width, o_).unsqueeze(2)).squeeze(2)      # [N, 9 Cout, H, width]
            n, c9, h, _ = p.shape
            p = p.view(n, 3, c9 // 3, h, width)
            g = p[:, 1].clone()
            g[..., 4:] += p[:, 0][..., :-4]
            if not last:
                g[..., :-4] += p[:, 2][..., 4:]
            out.append(g.contiguous())
        return out[0], out[1], off, off_col

    def _ds_sheared_first_layer(self, left, right, shift, ds, arithmetic=None):
        """``downsample`` = ds > 1 (features at ds times the volume's resolution, BuildCostVolume_cuda.cu:224-225: out[d,h,w] samples the
        right feature on row ds*h at x = ds*w - shift[d]) on uniformly spaced planes shift[d] = (m0 + d) / q is the sheared layer
        with q*ds phases (r6): index q*ds*w - m0 - d of the row-subsampled right feature upsampled by q alone; the
        left feature is subsampled in both directions.  Two phases (ds = 2, whole-pixel planes -- the sweep that covers cfg2's range
        at twice the resolution): the existing 3 x 7 layers with the feature itself in the upsampled image's place.  Four phases
        (ds = 2 with half-pixel planes, ds = 4 with whole-pixel planes): three 3 x 3 layers added 4 elements apart
        (_sheared_layer4) and the expand kernels' q = 4 instantiation.  Anything else returns None -> the materialised route."""
        conv, bn = self.conv1[0][0], self.conv1[0][1]
        nonneg, structure = self._shift_structure(shift)
        assert nonneg                              # reference __init__.py:12
        if structure is None or structure[0] * ds not in (2, 4):
            return None
        q_up, m0 = structure
        phases = q_up * ds
        n, c = left.size(0), left.size(1)
        h, w, d = left.size(2) // ds, left.size(3) // ds, shift.size(1)
        if w % 8 or w > 512:
            return None
        if phases == 2:
            if not self._sheared_fits(2, m0, d, w, False):
                return None
        else:
            _, wu4, _, _ = self._sheared_geometry4(m0, d, w)
            if 4 * ((wu4 + 3) // 4 * 4 + 16 + d) > 150 * 1024:
                return None
        st = self._x3_select(left.device, arithmetic)         # this route's one look at the split-mode state
        left_s = left[:, :, ::ds, ::ds].contiguous()
        right_r = right[:, :, ::ds, :].contiguous()          # rows ds*h; every input column
        plans = _factored_plans(conv, c)
        scale, bias = _folded_bn(bn, plans["plan"])
        prep = _Prep(plans, c, conv.weight, st, scale, bias)  # the 2D layers on the fp32 kernels
        self._left_planes(prep, left_s)
        if phases == 2:      # the 3 x 7 layers of q = 2 with the feature itself in the upsampled image's place
            g, gcol, off, off_col, _ = self._sheared_inputs(prep, right_r, 2, m0, d, w, up=1)
        else:
            g, gcol, off, off_col = self._sheared4_inputs(plans, conv.weight.detach()[:, c:], right_r, q_up, m0, d, w)
        planes = prep.planes
        return self._finish_first_layer(
            prep, (n, c, d, h, w), left.device, None, arithmetic, "ds_sheared_first_conv",
            lambda v1s, sc, bi: ops.sheared_expand_split(g, gcol, planes, sc, bi, v1s, phases, m0, off, off_col, ops.EPI_RELU, st["flag"]),
            lambda v: ops.sheared_expand(g, gcol, planes, scale, bias, v, phases, m0, off, off_col, ops.EPI_RELU))

    def _gn_sheared_first_layer(self, left, right, shift, arithmetic=None):
        """``GlobalStack(gn=True)`` on uniformly spaced disparity planes WITHOUT the 1.47 GB volume (r6): with one
        channel per group -- GroupNorm(32, 32), what convbn_3d(..., gn=True) builds for 32 channels, reference submodule.py:41-49 --
        the first layer's statistics are per (sample, channel) over the volume, which is what the sheared layer's statistics pass
        computes for a train-mode BatchNorm at batch 1 (snvc_sheared_expand_stats: the raw result is never stored).  Per sample:
        statistics, then the expand pass applies scale / shift + ReLU and writes the split pair the split-mode GroupNorm tail reads.
        Returns None when the call does not qualify (another spacing, rows the sheared kernels do not cover, split mode off)."""
        conv, norm = self.conv1[0][0], self.conv1[0][1]
        guard = self._gn_qualifies(left.device, arithmetic)
        if guard is None:
            return None
        nonneg, structure = self._shift_structure(shift)
        assert nonneg                              # reference __init__.py:12
        n, c, h, w = left.shape
        d = shift.size(1)
        if structure is None or not self._sheared_fits(structure[0], structure[1], d, w, True):
            return None
        q, m0 = structure
        prep = _Prep(_factored_plans(conv, c), c, conv.weight)      # the 2D layers on the fp32 kernels; no folded norm
        self._left_planes(prep, left)
        g, gcol, off, off_col, _ = self._sheared_inputs(prep, right, q, m0, d, w)
        planes = prep.planes
        b1 = x3_norm_bound(norm, plan_for(conv, "_x3", left.device))
        e1 = x3_exponent(b1)
        v1s = self._v1s((n, c, d, h, w), left.device)
        gam = norm.weight.detach() if norm.weight is not None else None
        bet = norm.bias.detach() if norm.bias is not None else None
        try:
            for i in range(n):                     # GroupNorm statistics are per sample
                sc, sh, _, _ = ops.sheared_expand_stats(g[i:i + 1], gcol[i:i + 1], planes[i:i + 1], gam, bet, (1, c, d, h, w), q, m0, off,
                                                        off_col, norm.eps)
                ops.sheared_expand_split(g[i:i + 1], gcol[i:i + 1], planes[i:i + 1], (sc * 2.0 ** e1).reshape(-1).contiguous(),
                                         (sh * 2.0 ** e1).reshape(-1).contiguous(), v1s[i:i + 1], q, m0, off, off_col, ops.EPI_RELU, guard.flag)
        except ops.Unsupported:
            return None
        _ROUTES["gn_sheared_first_conv"] += 1
        return self._gn_tail_x3(SplitT(v1s, e1, b1), None, arithmetic)

    def _conv2_tail(self, v1, shape, timing=None, arithmetic=None, st=_ASK):
        """Everything behind an fp32 first-layer result ``v1`` (from ``_v1``).  ``st``: the split-mode state the caller resolved for
        this step (None: fp32 arithmetic); left out, it is asked for here."""
        gn_cost = self._gn_tail_x3(v1, timing, arithmetic)
        if gn_cost is not None:
            return gn_cost
        if st is _ASK:
            st = self._x3_select(v1.device, arithmetic) if (v1.is_cuda and v1.dtype == torch.float32) else None
        if st is not None:      # split mode from an fp32 first-layer result: one layout pass (the sheared path writes the pair itself)
            return self._tail_x3(st, ops.to_split(v1, st["exp"]["v1"], out=self._v1s(v1.shape, v1.device, last="v1")), timing)
        _mark(timing, "conv2", 0)
        v, hv = self.conv2.fused(v1, out=self._buffer("v2", shape, v1.device), side_head=self.classifier)
        _mark(timing, "conv2", 1)
        return self._tail(v, hv)

    def forward(self, volume):
        from ..lazy import LazyCostVolume
        if isinstance(volume, LazyCostVolume):
            # build_cost_volume's result that nobody has looked at yet: the reference's call sequence on the fused path
            # ... or that somebody only PEEKED at (materialised, never written to: same values, so the fused path still applies)
            if volume.is_pristine and not torch.is_grad_enabled() and not self.training:
                left, right, shift, ds = volume.sources
                if left.shape[1] * 2 == self.conv1[0][0].in_channels and left.shape[3] % 4 == 0:
                    from .. import lazy as _lazy
                    _lazy.CONSUMER.ref = weakref.ref(self)      # the next build_cost_volume starts this model's first-layer prep
                    pre = volume.take_prefetch(self)
                    if pre is not None:                         # build_cost_volume already ran the step up to its host sync
                        def resume():
                            cost = _run(pre)
                            _ROUTES["lazy_prefetch_resumed"] += 1
                            return cost
                        return self.checked(self.arithmetic, resume, lambda: self._forward_pair_unchecked(
                            left, right, shift, ds, shift_checked=True, spacing=volume.spacing, arithmetic="fp32"))
                    return self.forward_pair(left, right, shift, ds, shift_checked=True, spacing=volume.spacing)
            # built from these two features: its maximum is theirs (interpolation weights are in [0, 1]), if they are untouched
            # ... and the volume itself: one that was written to in place (vol.mul_(8)) no longer has their maximum
            scale_from = tuple(volume.sources[:2]) if volume.is_pristine else None
            # the 1.47 GB volume is built and conv1 runs over all 64 channels (about half the pairs/s of the fused path): said once
            # per model, with the reason, and counted ("documented, not reported per call")
            _ROUTES["lazy_volume_materialized"] += 1
            if not self.__dict__.get("_snvc_lazy_warned"):
                self.__dict__["_snvc_lazy_warned"] = True
                why = ("autograd is enabled" if torch.is_grad_enabled() else "the model is in training mode" if self.training else
                       "the volume or its sources were written to after build_cost_volume" if not volume.is_pristine else
                       "the feature shape is outside the fused first layer's (2C input channels, W % 4 == 0)")
                warnings.warn("snvc_amd: model(build_cost_volume(...)) is taking the MATERIALISED route (the whole concat volume is built): "
                              + why + ".  forward_pair(left, right, shift) is the fused entry point.")
            return self._forward_volume(volume.materialize(), scale_from=scale_from)
        return self._forward_volume(volume)

    def lazy_prefetch(self, left, right, shift):
        """Called by ``build_cost_volume`` (no_grad, fp32, downsample 1) for the model that consumed the previous lazy volume: runs
        this call's step up to and including its one host sync -- the sign / spacing check of ``shift`` (reference __init__.py:12:
        an AssertionError for a negative shift comes out of build_cost_volume exactly as before) -- with the left half's planes
        and the speculative first-layer prep queued in front of the wait, and returns the paused generator (None if this model
        would not take the fused path for these inputs)."""
        conv, bn = self.conv1[0][0], self.conv1[0][1]
        if (self.training or torch.is_grad_enabled() or not isinstance(bn, nn.BatchNorm3d) or bn.training or left.device != conv.weight.device
                or left.shape[1] * 2 != conv.in_channels or left.shape[3] % 4 != 0 or shift.size(1) < 4 or shift.dtype != torch.float32
                or left.size(0) == 0 or left.dtype != torch.float32):
            return None                    # forward_pair would not reach the factored step, the one route with a pause point
        gen = self._factored_pair_steps(left, right, shift, pause=True)
        next(gen)
        return gen

    def _checked(self, fn, arithmetic, *args, **kw):
        """Run a split-mode capable entry point under ``SplitModePolicy.checked``: a flagged call is redone with arithmetic="fp32"."""
        return self.checked(arithmetic or self.arithmetic, lambda: fn(*args, arithmetic=arithmetic, **kw),
                            lambda: fn(*args, arithmetic="fp32", **kw))

    def _forward_volume(self, volume, timing=None, arithmetic=None, scale_from=None):
        return self._checked(self._forward_volume_unchecked, arithmetic, volume, timing=timing, scale_from=scale_from)

    def _forward_volume_unchecked(self, volume, timing=None, arithmetic=None, scale_from=None):
        """conv1 over a materialised [N, 2C, D, H, W] volume, then the tail.  Split mode (r4): the volume is scaled by a power of
        two derived on the device from its own maximum (or from the features it was built from, ``scale_from``: the volume holds
        nothing but their values and interpolations) and split once, conv1 runs on the split-mode kernel and writes the pair
        conv2 reads."""
        if torch.is_grad_enabled() or not volume.is_cuda:
            return self._tail(self.conv2(self.conv1(volume)))
        n, c2 = volume.size(0), volume.size(1)
        shape = (n, c2 // 2) + tuple(volume.shape[2:])
        splittable = volume.dtype == torch.float32 and c2 % 16 == 0
        gguard = self._gn_qualifies(volume.device, arithmetic) if splittable else None
        st = self._x3_select(volume.device, arithmetic) if splittable and gguard is None else None
        if gguard is not None or st is not None:      # the volume split once, conv1 and everything behind it in split mode
            mul = ops.split_scale_for(*(scale_from if scale_from is not None else (volume,)))
            vs = SplitT(ops.to_split(volume, mul_dev=mul, out=self._buffer("vol_s", (n, 2, c2 // 8) + tuple(volume.shape[2:]) + (8,),
                                                                             volume.device, torch.float16)), 0, None, mul)
        if gguard is not None:      # GroupNorm stack (r5)
            _mark(timing, "conv1", 0)
            v1s = self.conv1.fused_x3(vs, flag=gguard.flag)
            _mark(timing, "conv1", 1)
            return self._gn_tail_x3(v1s, timing, arithmetic)
        if st is not None:
            v1s = self._v1s(shape, volume.device)
            _mark(timing, "conv1", 0)
            self.conv1.fused_x3(vs, out=v1s, out_exp=st["exp"]["v1"], flag=st["flag"])
            _mark(timing, "conv1", 1)
            return self._tail_x3(st, v1s, timing)
        _mark(timing, "conv1", 0)
        v = self.conv1.fused(volume, out=self._v1(shape, volume.device))
        _mark(timing, "conv1", 1)
        return self._conv2_tail(v, shape, timing, arithmetic, st if splittable else _ASK)

    @staticmethod
    def _shift_structure(shift):
        """One device -> host round trip (it replaces the `assert torch.all(shift >= 0)` sync of the reference's wrapper):
        (all shifts >= 0, (q, m0) or None).  (q, m0): every row of ``shift`` is (m0 + d) / q for d = 0..D-1 with q in {1, 2}
        -- uniformly spaced whole- or half-pixel disparity planes -- exactly, in fp32."""
        return ops.shift_spacing_result(ops.shift_structure_begin(shift.detach()), shift.size(1))     # one launch (r3: 12 torch kernels, 60 us)

    @staticmethod
    def _sheared_fits(q, m0, d, w, training):
        """The limits of csrc/sheared_conv.hip's launchers (they return SNVC_ERR_UNSUPPORTED beyond them), mirrored so that
        such shapes take the general path instead of aborting the step: rows of at most 512 float4 pieces, and per workgroup
        one row block's window of G plus D plane offsets in <= 150 KB of LDS (inference: at least one row; the training
        kernels' own formulas: snvc_sheared_expand_stats like the forward, snvc_sheared_backward_reduce 4 rows of G, G',
        their sums and D)."""
        if w % 4 or w // 4 > 512:
            return False
        _, wu, _, wu_col = sheared_geometry(q, m0, d, w)
        lw = (wu + q - 1) // q + 4
        if 4 * (q * lw + d) > 150 * 1024:
            return False
        if training and 4 * 4 * (q * lw + d + 2 * wu + 2 * wu_col) > 150 * 1024:
            return False
        return True

    # ------------------------------------------------------------------------------- the first layer's weight folds and their layers
    @staticmethod
    def _layers(cache, key, kind, fold):
        """``cache[key]``: the depth-1 "same" layers of one weight fold, built once per weight.  ``fold()`` returns the folded
        [Cout', C, 3, kw] kernels; ``kind`` is what runs them: fp32 ``ops.Conv3dLayer`` or split-mode ``ops.Conv2dLayerX3``."""
        if key not in cache:
            def layer(k):
                k, kw = k.float().contiguous(), k.shape[3]
                return kind(k) if kind is ops.Conv2dLayerX3 else kind(k, kw, 1, kw // 2, 1, False, planar=True, ksize_h=3 if kw != 3 else 0)
            cache[key] = tuple(layer(k) for k in fold())
        return cache[key]

    def _sheared_layers(self, plans, w, c, q, kind=ops.Conv3dLayer):
        """The depth-1 3 x 7 layers that compute G and G' (csrc/sheared_conv.hip): K[kh][t] = sum over (kd, kw) with
        q*kw - kd = t of the right-half weights ``w[:, c:]``, folded in fp64; G' is the kernel without its kw = +1 taps."""
        def fold():
            k = sheared_kernels(w.detach()[:, c:], q)                      # [all | last column][depth class][Cout,C,3,7]
            return [k[i].reshape(3 * k.shape[2], k.shape[3], 3, 7) for i in range(2)]
        return self._layers(plans.setdefault("sheared" + _X3_KEY[kind], {}), q, kind, fold)

    @staticmethod
    def _left_planes_layer(plans, w, c, kind=ops.Conv3dLayer):
        """The three depth-class planes of the LEFT half of conv1(volume) as ONE depth-1 3x3 convolution of the left feature
        with 3*Cout output channels (channel co*3 + cls = the kd taps that class sees, summed in fp64): [N,3C,1,H,W] is
        the [N,C,3,H,W] tensor snvc_conv3d_forward_ex takes.  (r1-r2 ran the 3D kernel on the feature stacked 3 deep: a
        one-tile-deep launch whose time is one workgroup's whole channel loop, 50 us.)"""
        def fold():
            wl = w.detach()[:, :c].double()                                 # [Cout, C, kd, kh, kw]
            return [torch.stack([wl[:, :, 1:].sum(2), wl.sum(2), wl[:, :, :2].sum(2)], dim=1).reshape(-1, c, 3, 3)]      # [Cout, 3, C, kh, kw]
        return GlobalStack._layers(plans, "left2d" + _X3_KEY[kind], kind, fold)[0]

    @staticmethod
    def _left_planes_layer_cm(plans, w, c):
        """``_left_planes_layer``'s split-mode layer with its rows in class-major order (row cls * C + co holds channel co * 3 + cls):
        a lane's eight channels are then one channel group of the interleaved output.  Same fold, its own key, same validity rule."""
        def fold():
            wl = w.detach()[:, :c].double()
            k = torch.stack([wl[:, :, 1:].sum(2), wl.sum(2), wl[:, :, :2].sum(2)], dim=1).reshape(-1, c, 3, 3)
            return [k[torch.tensor(ops.class_major_rows(w.shape[0]), device=k.device)]]
        return GlobalStack._layers(plans, "left2d_cm_x3", ops.Conv2dLayerX3, fold)[0]

    @staticmethod
    def _commuted_weights(wr):
        """(P, Q, E) weights of the warp-after-convolution first layer as [*, C, 3, 3] depth-1 kernels (see _commuted_layers)."""
        w = wr.detach()                                                   # [Cout, C, kd, kh, kw]
        cout, c = w.shape[0], w.shape[1]
        wk = w.permute(2, 0, 1, 3, 4).contiguous()                        # [kd, Cout, C, kh, kw]
        kq = torch.zeros_like(wk)
        kq[..., 1] = wk[..., 2]
        ke = torch.zeros((3, 3, cout, c, 3, 3), dtype=w.dtype, device=w.device)
        for kw in range(3):
            ke[:, kw, :, :, :, 1] = wk[..., kw]
        return tuple(t.reshape(-1, c, 3, 3) for t in (wk, kq, ke))

    @staticmethod
    def _commuted_layers(plans, w, c, kind=ops.Conv3dLayer):
        """The depth-1 layers of the warp-after-convolution form of the first layer (csrc/sheared_conv.hip, any shift array):
        P_kd = conv2d(right, W[:, :, kd]); Q_kd = the kw = +1 taps alone (on the centre column); E[kd][kw] = the (c, kh)
        contraction with the kw taps, applied to the image's first column."""
        return GlobalStack._layers(plans, "commuted" + _X3_KEY[kind], kind, lambda: GlobalStack._commuted_weights(w.detach()[:, c:]))

    # ------------------------------------------------------------------------------------ the first layer's small 2D launches
    def _left_planes(self, prep, left):
        """Fills ``prep.planes`` ([N,C,3,H,W]: first / interior / last depth class of the left half) and, for the fused first layer,
        ``prep.p_il``: the same planes channel-interleaved, a second output of the same launch."""
        if prep.split_prep:     # one host call: the left feature's scale, its split pair, the 3x3 layer with 3 * Cout output channels
            lx = self._left_planes_layer(prep.plans, prep.weight, prep.c, ops.Conv2dLayerX3)
            if prep.fuse:
                planes, prep.p_il = ops.planes_x3_il(left, lx, prep.prep_ws.setdefault("planes_il", {}))
            else:
                planes = ops.conv2d_x3_from_f32(left, [lx], prep.prep_ws.setdefault("planes", {}))[0]
        else:
            planes = self._left_planes_layer(prep.plans, prep.weight, prep.c)(left.unsqueeze(2))   # [N,3C,1,H,W] ...
        prep.planes = planes.view(left.size(0), prep.c, 3, left.size(2), left.size(3))              # ... = [N,C,3,H,W]

    # (the two chains below on two side streams, joined by events before the expand pass, were built and measured in r5 with interleaved
    # legs: 2.185 ms/step against 2.130 on one stream -- the cross-stream event waits cost more than the chains' overlap buys.  Removed.)
    def _sheared_inputs(self, prep, right, q, m0, d, w, up=None, pool_left=None):
        """(G, G', off, off_col, il) of the sheared layer with q phases on D = ``d`` planes and rows of ``w``: the depth-1 3 x 7 layers on
        ``right`` upsampled by ``up`` (q unless the caller's feature already is the upsampled image).  ``il`` (fused first layer only):
        (G | G' channel-interleaved, pitch, lp).  ``pool_left`` (fused first layer, q = 1 | 2): the left feature whose planes the caller
        has NOT queued -- one pooled call (ops.prep_pooled_x3) then fills ``prep.planes`` and ``prep.p_il`` as ``_left_planes`` would."""
        off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
        if prep.split_prep:
            # r5: G and G' (depth-1 3 x 7 layers, 7.8 + 2.5 GFLOP: 84 + 31 us on the fp32 matrix pipe) in split mode like the layers behind
            # them: Rq is written as a split pair scaled by the right feature's own maximum (one launch, no host round trip)
            lx_g, lx_col = self._sheared_layers(prep.plans, prep.weight, prep.c, q, ops.Conv2dLayerX3)
            # one host call for the five launches (behind the step's host sync the GPU is empty: five Python-level launches of
            # 5-20 us kernels starve it); G / G' live in a per-model workspace until this call's expand pass has read them
            il = None
            if prep.fuse and q in (1, 2):      # G | G' also channel-interleaved, zero around the rows: what conv2's launch reads
                pitch, lp = ops.fused_il_geometry(q, m0, d, w, wu, off, wu_col, off_col)
                if pool_left is not None:
                    global POOLED_PREP_CALLS
                    cm = bool(self.planes_class_major)
                    lx = (self._left_planes_layer_cm(prep.plans, prep.weight, prep.c) if cm else
                          self._left_planes_layer(prep.plans, prep.weight, prep.c, ops.Conv2dLayerX3))
                    planes, prep.p_il, g, gcol, gi = ops.prep_pooled_x3(pool_left, right, q, wu, off, wu_col, off_col, lx_g, lx_col, lx,
                                                                        prep.prep_ws.setdefault("pooled", {}), pitch, lp, int(cm))
                    prep.planes = planes.view(right.size(0), prep.c, 3, right.size(2), right.size(3))
                    POOLED_PREP_CALLS += 1
                else:
                    g, gcol, gi = ops.sheared_prep_x3_il(right, q, wu, off, wu_col, off_col, lx_g, lx_col,
                                                         prep.prep_ws.setdefault("sheared_il", {}), pitch, lp)
                il = (gi, pitch, lp)
            else:
                g, gcol = ops.sheared_prep_x3(right, q, wu, off, wu_col, off_col, lx_g, lx_col, prep.prep_ws.setdefault("sheared", {}))
            _ROUTES["sheared_prep_x3"] += 1
            return g, gcol, off, off_col, il
        lay_g, lay_col = self._sheared_layers(prep.plans, prep.weight, prep.c, q)
        up = q if up is None else up
        g = lay_g(ops.sheared_upsample(right, up, wu, off).unsqueeze(2)).squeeze(2)                 # [N,3C,H,WU]
        gcol = lay_col(ops.sheared_upsample(right, up, wu_col, off_col).unsqueeze(2)).squeeze(2)    # [N,3C,H,WU2]
        return g, gcol, off, off_col, None

    def _commuted_inputs(self, prep, right):
        """(P, Q, E) of any other shift array: three 2D convolutions of the right feature (P, Q) and of its first columns (E)."""
        if prep.split_prep and (9 * prep.weight.shape[0]) % 32 == 0:
            # the three depth-1 3x3 layers in split mode: P and Q share the right feature's split pair (one host call), E runs on its
            # first four columns (another)
            lx_p, lx_q, lx_e = self._commuted_layers(prep.plans, prep.weight, prep.c, ops.Conv2dLayerX3)
            p_, q_ = ops.conv2d_x3_from_f32(right, [lx_p, lx_q], prep.prep_ws.setdefault("commuted", {}))
            e_ = ops.conv2d_x3_from_f32(right[:, :, :, :4], [lx_e], prep.prep_ws.setdefault("commuted_e", {}))[0]
            _ROUTES["commuted_prep_x3"] += 1
        else:
            lay_p, lay_q, lay_e = self._commuted_layers(prep.plans, prep.weight, prep.c)
            r5 = right.unsqueeze(2)
            p_, q_ = lay_p(r5).squeeze(2), lay_q(r5).squeeze(2)
            e_ = lay_e(right[:, :, :, :4].contiguous().unsqueeze(2)).squeeze(2)
        return p_, q_, e_

    def _finish_first_layer(self, prep, shape, device, timing, arithmetic, route, expand_split, expand):
        """The expand pass of a first layer of fp32 ``shape`` [N,C,D,H,W] and everything behind it.  Split mode: ``expand_split(v1s, scale,
        bias)`` writes the (hi, lo) pair conv2 reads (same bytes as the fp32 tensor, no layout pass); otherwise, or when that launcher
        says ``Unsupported``, ``expand(v)`` writes the fp32 tensor.  Counts ``route``.  None: both said ``Unsupported`` (a limit
        _sheared_fits does not mirror, rows that do not fit the LDS): the caller's next route gives the same answer."""
        st = prep.st
        if st is not None and prep.c % 8 == 0:
            v1s = self._v1s(shape, device)
            try:
                expand_split(v1s, *self._x3_v1_affine(st, prep.scale, prep.bias))
            except ops.Unsupported:
                pass
            else:
                _mark(timing, "conv1", 1)
                _ROUTES[route] += 1
                return self._tail_x3(st, v1s, timing)
        v = self._v1(shape, device)
        try:
            expand(v)
        except ops.Unsupported:
            return None
        _mark(timing, "conv1", 1)
        _ROUTES[route] += 1
        return self._conv2_tail(v, shape, timing, arithmetic, st)

    # -------------------------------------------------------------------------------------------------------- forward_pair
    def forward_pair(self, left, right, shift, downsample=1, factored=True, timing=None, shift_checked=False, sheared=True,
                     fused_bn=True, spacing="unknown", commuted=True, arithmetic=None):
        return self._checked(self._forward_pair_unchecked, arithmetic, left, right, shift, downsample, factored, timing, shift_checked,
                             sheared, fused_bn, spacing, commuted)
    forward_pair.__doc__ = "see _forward_pair_unchecked"

    def _forward_pair_unchecked(self, left, right, shift, downsample=1, factored=True, timing=None, shift_checked=False, sheared=True,
                                fused_bn=True, spacing="unknown", commuted=True, arithmetic=None):
        """cost-volume build + 3D CNN forward: the unit BASELINE.json's metric counts.  This function only picks the route, in this
        order: training (_train_pair), the downsample 2 / 4 sheared layer, the GroupNorm sheared layer, the materialised volume
        (_materialised_pair), the factored inference step (_factored_pair_steps).

        ``factored=True`` (inference, eval BatchNorm, downsample 1) uses the structure of the CONCAT
        volume: its left half repeats the left feature on every disparity plane
        (BuildCostVolume_cuda.cu:86), so the left half of conv1(volume) does not depend on d except
        at the two zero-padded ends.  It is computed once as three depth-class planes (this same
        conv kernel on the left feature stacked 3 deep with conv1's left-half weights) and added in
        the epilogue of the 3D convolution over the RIGHT half only -- which is also the only half
        of the volume that has to be built.  Same result (fp32 summation order aside), half of
        conv1's work and of the volume's HBM traffic.  ``factored=False`` materialises the full volume
        through ``build_cost_volume`` exactly like the reference would.
        ``sheared=True`` (with ``factored``): when the disparity planes are uniformly spaced by a whole or half pixel --
        ``shift[n, d] = (m0 + d) / q``, q in {1, 2}, what a plane sweep over disparities is (BASELINE.json configs[1]:
        linspace(0, 95.5, 192)) -- the warped half is a shear of ONE 2D image and conv1 over it is a 2D convolution
        evaluated along the shear (csrc/sheared_conv.hip): the warped volume is not built at all and conv1's 318 GFLOP
        become 3.4.  Any other shift array (checked on the device, same sync as the reference's assert) takes the
        general factored path.
        ``arithmetic``: None (the model's ``arithmetic`` attribute, default "auto"), "fp32" or "x3": whether conv2 and the
        hourglass run on the split-mode kernels (see ``_x3_state``).
        ``timing``: optional dict ``{"volume": (start, end), "conv1": (start, end)}`` of events recorded on the
        current stream around the cost-volume launch and the first 3D convolution (the dominant kernel); used by
        bench.py for the roofline figures."""
        conv, bn = self.conv1[0][0], self.conv1[0][1]
        n, c, h, w = left.shape
        d = shift.size(1)
        grad = torch.is_grad_enabled()
        if (grad and (left.requires_grad or right.requires_grad or conv.weight.requires_grad) and factored and timing is None
                and downsample == 1 and left.dtype == torch.float32 and w % 4 == 0 and (h * w) % 4 == 0 and d >= 2):
            return self._train_pair(left, right, shift, sheared, fused_bn, commuted)
        # The inference gates.  Every route asks for `infer`; eval-mode BatchNorm is what folds into a scale and a bias.
        infer = factored and not grad and left.dtype == torch.float32
        bn_eval = isinstance(bn, nn.BatchNorm3d) and not bn.training
        # The two special sheared layers have no general form behind them, so they also ask up front for what the factored step checks on
        # its way or leaves to its fallbacks (a device, a float32 array of D >= 4 for the spacing kernel, a sample, split-pair channels),
        # and they take no `timing`: their launches are not the brackets' launches.
        special = (infer and sheared and timing is None and left.is_cuda and d >= 4 and shift.dtype == torch.float32 and n > 0
                   and c % 8 == 0 and c * 2 == conv.in_channels)
        # left.shape == right.shape: only this route strides both features itself, in front of every launcher that would compare them
        if special and bn_eval and downsample in (2, 4) and h % downsample == 0 and w % downsample == 0 and left.shape == right.shape:
            cost = self._ds_sheared_first_layer(left, right, shift, downsample, arithmetic)      # r6; None: the materialised route below
            if cost is not None:
                return cost
        # W % 8, W <= 512: the statistics pass's row limits.  The downsample route asks them of its subsampled rows (inside); the factored
        # step's expand kernels need W % 4 alone (below, _sheared_fits)
        if (special and downsample == 1 and not self.training and isinstance(bn, nn.GroupNorm) and bn.num_groups == conv.out_channels
                and w % 8 == 0 and w <= 512):
            cost = self._gn_sheared_first_layer(left, right, shift, arithmetic)       # r6; None: the paths below
            if cost is not None:
                return cost
        if not (infer and bn_eval and downsample == 1 and w % 4 == 0 and d >= 2):
            return self._materialised_pair(left, right, shift, downsample, timing, arithmetic)
        return _run(self._factored_pair_steps(left, right, shift, timing, shift_checked, sheared, spacing, commuted, arithmetic))

    def _train_pair(self, left, right, shift, sheared, fused_bn, commuted):
        """Training (cfg4): the same factoring with a backward pass (half the first layer's dgrad / wgrad, no 1.5 GB volume)."""
        conv, bn = self.conv1[0][0], self.conv1[0][1]
        structure = None
        if sheared and left.size(0) > 0 and shift.size(1) >= 4 and shift.dtype == torch.float32 and left.size(1) <= 32:
            nonneg, structure = self._shift_structure(shift)
            assert nonneg
        else:
            assert torch.all(shift >= 0.)
        plan = plan_for(conv, "", left.device)
        if structure is not None and not self._sheared_fits(structure[0], structure[1], shift.size(1), left.size(3), True):
            structure = None           # rows the sheared kernels do not cover (csrc/sheared_conv.hip's LDS limits): general path
        if (structure is not None and isinstance(bn, nn.BatchNorm3d) and bn.training and left.size(3) % 8 == 0
                and left.size(3) <= 512 and fused_bn):
            # ... with train-mode BatchNorm + ReLU folded around it: neither the raw result nor its gradient is ever stored
            v = _ShearedFirstConvBNFn.apply(left, right, conv.weight, bn.weight, bn.bias, conv, bn, plan, structure[0], structure[1],
                                            shift.size(1))
        elif structure is not None:      # uniformly spaced planes: the sheared 2D form, forward and backward
            v = _ShearedFirstConvFn.apply(left, right, conv.weight, bn.weight, bn.bias, conv, bn, EPI_RELU, plan, structure[0],
                                          structure[1], shift.size(1))
        else:
            v = _FactoredFirstConvFn.apply(left, right, shift, conv.weight, bn.weight, bn.bias, conv, bn, EPI_RELU, plan, commuted)
        return self._tail(self.conv2(v))

    def _materialised_pair(self, left, right, shift, downsample, timing, arithmetic):
        """The whole concat volume, then the modules: what the reference does.  With ``timing`` the volume is built by the launcher itself,
        so that the event pair holds that launch alone."""
        if timing is None:
            vol = _BuildCostVolume.apply(left, right, shift, downsample)      # the eager volume
            if torch.is_grad_enabled() or not vol.is_cuda:
                return self.forward(vol)
            return self._forward_volume(vol, None, arithmetic, scale_from=(left, right) if downsample == 1 else None)
        assert torch.all(shift >= 0.)        # the wrapper's own check (a sync) stays outside the event pair
        _mark(timing, "volume", 0)
        vol = ops.cost_volume_forward(left, right, shift, downsample)
        _mark(timing, "volume", 1)
        if torch.is_grad_enabled():
            _mark(timing, "conv1", 0)
            v = self.conv1(vol)
            _mark(timing, "conv1", 1)
            del vol
            return self._tail(self.conv2(v))
        return self._forward_volume(vol, timing, arithmetic, scale_from=(left, right))

    def _factored_pair_steps(self, left, right, shift, timing=None, shift_checked=False, sheared=True, spacing="unknown", commuted=True,
                             arithmetic=None, pause=False):
        """The factored inference step (eval BatchNorm, downsample 1, float32 features with W % 4 == 0, D >= 2), as a GENERATOR: with
        ``pause`` it yields once, right after the step's host sync (the shift array's sign / spacing check) with the left half's planes
        and the speculative first-layer prep already queued -- ``build_cost_volume`` runs it up to there for the model that consumed
        the last lazy volume (the reference's `assert` fires at build time as before, and the GPU is not left idle while the host
        waits), ``GlobalStack.forward`` resumes it.  Without ``pause`` it runs straight through.  The generator's return value is the
        cost tensor.  Behind the sync: the sheared layer, else warp-after-convolution, else the right half built."""
        conv, bn = self.conv1[0][0], self.conv1[0][1]
        c, d, w = left.size(1), shift.size(1), left.size(3)
        # The one device -> host sync of the step (the wrapper's `assert shift >= 0`, here also the shift array's spacing) is
        # STARTED first and awaited only after everything that does not need its answer has been queued: the left half's
        # planes, and -- speculatively, for the spacing the previous call saw -- the sheared layer's two small 2D convolutions.
        # The host then waits while the GPU still has work, and queues the big layers while those run (r3: the wait sat in
        # front of six small launches whose launch latency the GPU then had to sit through, ~0.1 ms of a 4 ms step).
        ticket = None
        known = shift_checked and spacing != "unknown"       # build_cost_volume already looked (LazyCostVolume.spacing)
        if known and not sheared:
            spacing = None
        if not known and left.size(0) > 0 and d >= 4 and shift.dtype == torch.float32:
            # (r5: also with sheared=False -- the sign check rides on the same launch instead of a blocking torch.all in front of
            # an empty queue: 93 us of idle GPU per step on the any-shift path)
            ticket = ops.shift_structure_begin(shift.detach())
        elif not shift_checked:                  # a LazyCostVolume was checked when build_cost_volume made it
            assert torch.all(shift >= 0.)
        plans = _factored_plans(conv, c)
        scale, bias = _folded_bn(bn, plans["plan"])
        # the step's one look at the split-mode state (a paused step looks again when it goes on): it cannot change before the tail, where
        # guard.post() is, so everything below is handed it
        st = self._x3_select(left.device, arithmetic)
        # the first layer's small 2D convolutions run in split mode whenever the stack behind them does (same arithmetic contract:
        # fp32 accuracy on the half pipe); `arithmetic="fp32"` keeps every layer on the fp32-MFMA kernels
        split_prep = bool(st is not None and self.split_prep and c % 8 == 0 and (3 * conv.out_channels) % 32 == 0 and right.is_contiguous()
                          and (not left.is_contiguous() or left.data_ptr() % 16 == 0) and right.data_ptr() % 16 == 0)     # the scale launch reads float4
        # the fused first layer (fused_first) reads the planes and G | G' channel-interleaved
        fuse = bool(split_prep and self.fused_first and sheared and conv.out_channels == c and left.size(0) > 0
                    and st["layers"]["conv2"].fused_first_form(left.size(0), (d,) + tuple(left.shape[2:])))
        # r6: the prep results (planes, G / G', P / Q / E) live in per-model buffers that the NEXT call through here overwrites.  Every
        # call takes a new epoch; a step that was paused (build_cost_volume's speculative start) compares it when it is resumed
        # (a process-wide counter: invalidate_plans(model) drops the attribute, and a fresh count must not meet an old step's number)
        epoch = self.__dict__["_snvc_prep_epoch"] = next(_PREP_EPOCH)
        prep = _Prep(plans, c, conv.weight, st, scale, bias, split_prep, fuse, self.__dict__.setdefault("_snvc_prep_ws", {}))
        can_commute = commuted and shift.dtype == torch.float32 and w <= 2048
        structure, guess, ready, ready_general = (spacing if known else None), None, None, None
        if ticket is not None:
            guess = plans.get("spacing_seen")    # (q, m0, D, W) of the previous call, or ("general", D, W): a guess, checked below
        guessed = ticket is not None and sheared and guess is not None and guess[0] != "general" and guess[2:] == (d, w)   # a guess for this shape
        # pooled_prep: where the fused first layer's sheared inputs are queued anyway -- the spacing is known, or guessed for this shape --
        # the left planes are not queued on their own: the first _sheared_inputs below fills them too, three launches for the eight.
        # In every other case the planes go first, as they always did.
        pool_for = structure if known else (guess[:2] if guessed else None)
        pool_left = left if (fuse and self.pooled_prep and pool_for is not None and pool_for[0] in (1, 2) and left.shape == right.shape
                             and self._sheared_fits(pool_for[0], pool_for[1], d, w, False)) else None
        if pool_left is None:
            self._left_planes(prep, left)
        if ticket is not None:
            _mark(timing, "volume", 0)
            if guessed:
                ready = self._sheared_inputs(prep, right, guess[0], guess[1], d, w, pool_left=pool_left)
                pool_left = None                 # the planes are queued: a wrong guess re-runs the sheared inputs alone
            elif can_commute and (not sheared or (guess is not None and guess[0] == "general" and guess[1:] == (d, w))):
                ready_general = self._commuted_inputs(prep, right)
            nonneg, structure = ops.shift_spacing_result(ticket, d)
            assert nonneg                        # same contract as build_cost_volume (reference __init__.py:12)
            if sheared:
                plans["spacing_seen"] = structure + (d, w) if structure is not None else ("general", d, w)
            else:
                structure = None                 # the caller asked for the general path
        if pause:
            yield "shift checked; planes and speculative prep queued"
            # resumed by GlobalStack.forward(volume).  Anything may have run on this model in between -- another build_cost_volume (two
            # pending volumes), a forward_pair, a parameter update: if the prep buffers are no longer this step's own, or the folded
            # first-layer parameters moved, the step starts over from its inputs (the shift array's answer stays: it was checked)
            if not (self.__dict__.get("_snvc_prep_epoch") == epoch and conv.__dict__.get("_snvc_factored") is plans
                    and fresh(plans["stamp"], (conv.weight,)) and all(a is b for a, b in zip(_folded_bn(bn, plans["plan"]), (scale, bias)))):
                _ROUTES["lazy_prefetch_stale"] += 1
                return self._forward_pair_unchecked(left, right, shift, 1, True, timing, True, sheared, True, structure, commuted, arithmetic)
            # ... and the layers behind the first one are those of the moment the step goes on (conv2's weight is in no key above): the
            # split-mode state is looked up again, the 2D launches queued before the pause stay as they were decided
            prep.st = self._x3_select(left.device, arithmetic)
        if structure is not None and not self._sheared_fits(structure[0], structure[1], d, w, False):
            structure = None                     # rows the sheared kernels do not cover: the paths below
        if pool_left is not None and structure is None:
            self._left_planes(prep, left)        # nothing below queues the sheared inputs after all: the planes on their own
            pool_left = None
        cost = None
        if structure is not None:
            if ready is None or tuple(guess[:2]) != tuple(structure):
                _mark(timing, "volume", 0)
                # first call, or the spacing changed: the guess is dropped (pool_left: the spacing was known, nothing is queued yet)
                ready = self._sheared_inputs(prep, right, structure[0], structure[1], d, w, pool_left=pool_left)
            cost = self._sheared_pair(prep, ready, structure, (left.size(0), c, d) + tuple(left.shape[2:]), timing, arithmetic)
        if cost is None and can_commute:
            if ready_general is None:
                _mark(timing, "volume", 0)
                ready_general = self._commuted_inputs(prep, right)
            cost = self._commuted_pair(prep, ready_general, shift, timing, arithmetic)
        if cost is None:
            cost = self._right_half_pair(prep, left, right, shift, timing, arithmetic)
        return cost

    def _sheared_pair(self, prep, ready, structure, shape, timing, arithmetic):
        """Uniformly spaced planes: the expand pass over G / G' and the left planes, or (fused first layer) nothing at all here."""
        (q, m0), (g, gcol, off, off_col, il), st, planes = structure, ready, prep.st, prep.planes
        _mark(timing, "volume", 1)
        _mark(timing, "conv1", 0)
        if st is not None and il is not None:
            # the fused first layer: nothing runs here -- conv2's launch (the "conv2" marks) forms the pair itself
            _mark(timing, "conv1", 1)
            _ROUTES["sheared_first_conv"] += 1
            v1_sc, v1_bi = self._x3_v1_affine(st, prep.scale, prep.bias)

            def expand(t):      # last_first_layer(): the pair, from the operands this call leaves in the prep workspace
                ops.sheared_expand_split(g, gcol, planes, v1_sc, v1_bi, t, q, m0, off, off_col, ops.EPI_RELU, None)
                return t
            self._v1s(shape, g.device, lazy=expand)
            return self._tail_x3(st, None, timing, fused=(shape, g.device, dict(
                gi=il[0], pitch=il[1], lp=il[2], p_il=prep.p_il, v_scale=v1_sc, v_bias=v1_bi, q=q, m0=m0, off=off, off_col=off_col,
                v_flags=ops.EPI_RELU)))
        flags = ops.EPI_RELU | (ops.EPI_STREAM_OUT if self.stream_out else 0)
        return self._finish_first_layer(
            prep, shape, g.device, timing, arithmetic, "sheared_first_conv",
            lambda v1s, sc, bi: ops.sheared_expand_split(g, gcol, planes, sc, bi, v1s, q, m0, off, off_col, flags, st["flag"]),
            lambda v: ops.sheared_expand(g, gcol, planes, prep.scale, prep.bias, v, q, m0, off, off_col, ops.EPI_RELU))

    def _commuted_pair(self, prep, ready, shift, timing, arithmetic):
        """Any other shift array: interpolation along w commutes with the convolution -- three 2D convolutions of the right
        feature, three interpolations per output voxel, the warped volume is not built either (csrc/sheared_conv.hip).  None: rows
        that do not fit the LDS (grows with D): the right half is built instead."""
        (p_, q_, e_), st, planes = ready, prep.st, prep.planes
        _mark(timing, "volume", 1)
        _mark(timing, "conv1", 0)
        flags = ops.EPI_RELU | (ops.EPI_STREAM_OUT if self.stream_out else 0)
        shape = (planes.size(0), prep.c, shift.size(1)) + tuple(planes.shape[3:])
        return self._finish_first_layer(
            prep, shape, planes.device, timing, arithmetic, "commuted_first_conv",
            lambda v1s, sc, bi: ops.warped_expand_split(p_, q_, e_, planes, shift, sc, bi, v1s, flags, st["flag"]),
            lambda v: ops.warped_expand(p_, q_, e_, planes, shift, prep.scale, prep.bias, v, ops.EPI_RELU))

    def _right_half_pair(self, prep, left, right, shift, timing, arithmetic):
        """The warped right half built, the factored 3D convolution over it with the left planes added in its epilogue (r2's path)."""
        shape = (left.size(0), prep.c, shift.size(1)) + tuple(left.shape[2:])
        _mark(timing, "volume", 0)
        try:
            vol_r = ops.cost_volume_forward_right(right, shift, out=self._buffer("vol_r", shape, left.device))   # [N,C,D,H,W]
        except ops.Unsupported:                  # rows beyond the row builder's width: the materialised volume, as the reference
            return self.forward_pair(left, right, shift, 1, factored=False, timing=timing, arithmetic=arithmetic)
        _mark(timing, "volume", 1)
        _mark(timing, "conv1", 0)
        v = prep.plans["right"](vol_r, prep.scale, prep.bias, None, ops.EPI_RELU, self._v1(shape, left.device), depth_planes=prep.planes)
        _mark(timing, "conv1", 1)
        return self._conv2_tail(v, shape, timing, arithmetic, prep.st)

