"""Guard bands (tests/guarded.py) around the fp32 convolutions of conv3d.hip / conv3d_small.hip and the weight gradients of
conv3d_bwd.hip.

Every case is an existing test of the suite, imported and run unchanged twice: once in torch's own memory, once inside
``guarded(place_results=True)``, where each of its device tensors is an operand placed in the arena between NaN guards and each output,
workspace and packed-weight buffer the wrappers allocate lies between guard zones -- both times with the operands 256-byte aligned, and
both times again with them 4 bytes off that (8 for the cases whose rows are 8-byte pieces), so that the two runs take the same kernel forms.
Asserted (``guarded.run_case``): the guards are intact; every tensor a factory allocated is bit-equal to the unguarded run's; no
allocation on the device fell through; and the existing test's own assertions hold the guarded run to its reference at its tolerance.
"""
import numpy as np
import pytest
import torch

import guarded as GD
import test_gpu_parity as TP
import wgrad_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = "test_gpu_parity"
WF = "test_gpu_wgrad_forms"


def plain_conv_case(n, cin, cout, shape, k, stride, transposed=False):
    """Shapes the forward tests of the suite do not hold: a HipConv3d / HipConvTranspose3d layer against torch's float64 convolution on
    the CPU at test_gpu_parity's TIGHT, plain and with relu(conv + residual)."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    from test_gpu_parity import TIGHT, check
    r = np.random.default_rng(17 + cin + cout + shape[2])
    conv = S.HipConv3d(cin, cout, k, stride, k // 2, bias=False)
    w = torch.from_numpy((r.standard_normal(tuple(conv.weight.shape)) * 0.1).astype(np.float32))
    conv.weight.data.copy_(w)
    conv = conv.to(DEV)
    x = torch.from_numpy(r.standard_normal((n, cin) + shape).astype(np.float32))
    ref = F.conv3d(x.double(), w.double(), None, stride, k // 2)
    res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
    with torch.no_grad():
        check(conv(x.to(DEV)).cpu().numpy(), ref.numpy(), TIGHT, "plain")
        y = conv.fused(x.to(DEV), relu=True, residual=res.to(DEV))
        check(y.cpu().numpy(), F.relu(ref + res.double()).numpy(), TIGHT, "relu(conv+res)")


def fused_routes_case():
    """The fused entry points whose existing tests assert the fused route -- side head, avgpool fusion, deconv head, statistics epilogue
    -- held to references that do not care which route ran (torch on the CPU at TIGHT; the plain launch's bits; norm_stats over it at
    the statistics test's 2e-6 / 2e-7): with operands off 16 bytes the wrappers fall back to separate launches, and those run here."""
    import torch.nn.functional as F
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    from test_gpu_parity import TIGHT, check, seeded
    r = np.random.default_rng(77)
    t = lambda *shape: torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    bn = lambda y, b: F.batch_norm(y, b.running_mean.cpu(), b.running_var.cpu(), b.weight.cpu(), b.bias.cpu(), False, 0.0, b.eps)
    with torch.no_grad():
        head = S.HipConv3d(32, 1, kernel_size=1, padding=0, stride=1, bias=False)
        head.weight.data.copy_(t(1, 32, 1, 1, 1))
        hd = head.to(DEV)
        m = S.ConvBNReLU3d(seeded(S.convbn_3d(32, 32, 3, 1, 1), 392), torch.nn.ReLU(inplace=True)).to(DEV)
        x = t(2, 32, 5, 6, 40).to(DEV)
        plain = m.fused(x)
        y, hy = m.fused(x, side_head=hd)
        assert torch.equal(y, plain)
        check(hy.cpu().numpy(), F.conv3d(plain.cpu(), hd.weight.cpu()).numpy(), TIGHT, "side head")
        m2 = seeded(S.convbn_3d(64, 32, 3, 1, 1), 492).to(DEV)
        x2 = t(2, 64, 8, 6, 40)
        exp = F.avg_pool3d(F.relu(bn(F.conv3d(x2, m2[0].weight.cpu(), None, 1, 1), m2[1])), (4, 1, 1), (4, 1, 1))
        check(S.fused_conv3d_avgpool_d4(m2[0], m2[1], x2.to(DEV), relu=True).cpu().numpy(), exp.numpy(), TIGHT, "conv + avgpool")
        m3 = seeded(S._deconvbn_3d(64, 32, gn=False), 92).to(DEV)
        x3, res = t(2, 64, 3, 5, 34), t(2, 32, 6, 10, 68)
        exp = F.conv3d(F.relu(bn(F.conv_transpose3d(x3, m3[0].weight.cpu(), None, 2, 1, 1), m3[1]) + res), hd.weight.cpu())
        check(m3.fused(x3.to(DEV), relu=True, residual=res.to(DEV), head=hd).cpu().numpy(), exp.numpy(), TIGHT, "deconv + head")
        for cin, cout, stride, shape, transposed in ((6, 64, 1, (5, 7, 72), False), (4, 32, 2, (10, 14, 72), False), (6, 64, 2, (3, 5, 36), True)):
            w = (0.1 * t(*((cin, cout) if transposed else (cout, cin)), 3, 3, 3)).to(DEV)
            xs, gamma, beta = t(2, cin, *shape).to(DEV), (torch.rand(cout) + 0.5).to(DEV), t(cout).to(DEV)
            layer = ops.Conv3dLayer(w, 3, stride, 1, 1, transposed)
            got = layer.forward_stats(xs, gamma, beta, 1e-5)
            ref = layer(xs)
            conv = F.conv_transpose3d(xs.cpu(), w.cpu(), None, 2, 1, 1) if transposed else F.conv3d(xs.cpu(), w.cpu(), None, stride, 1)
            check(ref.cpu().numpy(), conv.numpy(), TIGHT, f"statistics layer {cin}->{cout}")
            want = ops.norm_stats(ref, gamma, beta, cout, False, 1e-5)
            if got is not None:              # None: the caller runs exactly the two launches above
                assert torch.equal(got[0], ref)
                for a_, b_ in zip(got[1:], want):
                    np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), rtol=2e-6, atol=2e-7)
            assert (got is None) == bool(xs.data_ptr() % 16), "the statistics epilogue runs exactly on 16-byte aligned inputs here"


# (id, module, function, keyword arguments, second placement in bytes).  8: the transposed kernels ask for 8-byte aligned y / residual
# and the entry point refuses anything else.  None: aligned only -- the wrapper falls back to another route for operands off 16 bytes
# (fused head, side head, avgpool fusion, statistics epilogue, the k1 streaming weight gradient), and the existing test asserts that
# the fused route was taken; ``fused_routes_case`` runs those entry points at both placements against references that hold either way.
ARENA = {"wgrad_k57": 2 << 30,          # the generic tap-chunk form's workspace query: 1.4 GB of per-workgroup partials for this k7 layer
         "wgrad_columns_s1": 256 << 20, "wgrad_columns_s2": 256 << 20}      # 57 MB of partials beside operands of up to 34 MB
CASES = []
for mode in ("default", "big", "std", "narrow", "direct"):               # (2, 32->32, (5, 7, W)) and (2, 6->64, (2, 9, W)), three epilogues
    CASES += [(f"k3_{mode}_W72", P, "test_k3_kernel_variants_vs_torch", dict(mode=mode, W=72), 4),
              (f"k3_{mode}_W78", P, "test_k3_kernel_variants_vs_torch", dict(mode=mode, W=78), 8)]
CASES.append(("k3_scalar_staging", __name__, "plain_conv_case", dict(n=2, cin=32, cout=32, shape=(3, 6, 37), k=3, stride=1), 4))
for form in ("slice_pipelined", "per_chunk"):                             # both refill forms, direct, direct + generic epilogue
    CASES += [(f"k3s2_{form}_W{W}", P, "test_k3_stride2_winograd_vs_torch", dict(W=W, form=form), 4) for W in (40, 44)]
CASES.append(("k3s2_odd_extents", __name__, "plain_conv_case", dict(n=2, cin=32, cout=64, shape=(5, 7, 41), k=3, stride=2), 4))
for k, dil in ((5, 1), (5, 2), (7, 1)):                                   # Winograd and exact=True
    CASES += [(f"k{k}d{dil}_W{W}", P, "test_k5_k7_winograd_vs_torch", dict(k=k, dil=dil, W=W), 4) for W in (24, 44)]
CASES += [
    ("transposed", P, "test_deconv_vs_torch", {}, 8),                                      # (2, 64->32, (3, 4, 33)), (2, 8->5, (1, 1, 1))
    ("k1", __name__, "plain_conv_case", dict(n=1, cin=40, cout=32, shape=(3, 5, 36), k=1, stride=1), 4),
    ("cin1", __name__, "plain_conv_case", dict(n=3, cin=1, cout=32, shape=(4, 4, 32), k=1, stride=1), 4),
    ("cout1_cout27_slices", P, "test_conv3d_epilogue_variants_and_slices", {}, 4),
    ("fused_head", P, "test_deconv_fused_head_vs_separate_layers", {}, None),
    ("side_head", P, "test_side_head_vs_separate_projection", {}, None),
    ("avgpool_d4_fusion", P, "test_conv_avgpool_d4_fused_vs_separate", {}, None),
    ("deconv_to_one_channel", P, "test_deconv_to_one_channel_vs_torch", {}, 8),
    ("fused_routes", __name__, "fused_routes_case", {}, 8),                 # 8: it holds a transposed layer with a residual
]
CASES += [(f"stats_{c}", P, "test_conv_statistics_epilogue_vs_separate_pass", dict(case=c), 4 if c == "unsupported_w78" else None)
          for c in TP.test_conv_statistics_epilogue_vs_separate_pass.pytestmark[0].args[1]]           # every name of its table

# ------------------------------------------------------------------------------------------------------------------- weight gradients
for c in ("k3s2 rows of 8 bytes", "k3s2 odd extents", "k1", "k1 to one channel", "k3 ragged"):
    CASES += [(f"wgrad_{c.replace(' ', '_')}_{v}", P, "test_conv3d_wgrad_vs_float64", dict(case=c, variant=v), 8 if "8 bytes" in c else 4)
              for v in ("auto", "fp32", "direct")]
CASES += [
    ("wgrad_k57", WF, "test_generic_tap_chunk_kernel_vs_float64", dict(case="k7 8-byte rows, partial blocks", variant="auto"), 8),
    ("wgrad_role_swap", WF, "test_role_swapped_call_vs_float64_transposed", dict(case="40->24 rows of 18", variant="auto"), 4),
    ("wgrad_depth1", WF, "test_depth_one_vs_float64", dict(case="k3s2 d1 odd channels", variant="auto"), 4),
    ("wgrad_dparts", WF, "test_depth_parts_vs_float64", dict(case="k3 D33"), 4),
    ("wgrad_strided", WF, "test_batch_strided_operands", dict(case="k3 unaligned", variant="auto"), 4),
    ("wgrad_columns_s1", WF, "test_column_limit_cases_vs_float64", dict(case="k3 257 columns", variant="auto"), 4),
    ("wgrad_columns_s2", WF, "test_column_limit_cases_vs_float64", dict(case="k3s2 513 columns", variant="auto"), 4),
    ("wgrad_k1_stream", WF, "test_k1_streaming_form_vs_float64", dict(case="k1 idle channels"), None),
    ("wgrad_maxima_s1", "test_gpu_wgrad_x3", "test_wgrad_with_supplied_maxima", dict(stride=1, shape=(2, 40, 24, (5, 10, 44)), slack=1.0), 4),
    ("wgrad_maxima_s2", "test_gpu_wgrad_x3", "test_wgrad_with_supplied_maxima", dict(stride=2, shape=(1, 32, 64, (6, 12, 40)), slack=1.0), 4),
]
assert all(c in WC.K57_CASES or c in WC.ROLE_SWAP_CASES or c in WC.DEPTH1_CASES or c in WC.DPART_CASES or c in WC.STRIDED_CASES
           or c in WC.K1_STREAM_CASES or c in WC.COLUMN_LIMIT_CASES
           for c in ("k7 8-byte rows, partial blocks", "40->24 rows of 18", "k3s2 d1 odd channels", "k3 D33", "k3 unaligned", "k1 idle channels",
                     "k3 257 columns", "k3s2 513 columns"))


RUNS = [(c, off) for c in CASES for off in (0, c[4]) if off is not None]


@pytest.mark.parametrize("case,off", RUNS, ids=[f"{c[0]}-{'aligned' if not off else 'off%d' % off}" for c, off in RUNS])
def test_guarded(case, off):
    key, module, name, kwargs, _ = case
    GD.run_existing(module, name, kwargs, DEV, off, **({"arena_bytes": ARENA[key]} if key in ARENA else {}))
