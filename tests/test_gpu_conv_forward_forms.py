"""Every kernel form of the fp32 forward convolution on the device, one small case per form and epilogue variant
(tests/conv_forward_cases.py).  Each case places its operands as the row says -- inside larger buffers that hold a fill value, at
the row's byte offset from a 256-byte boundary and with the row's batch-stride padding --, asks the library for the real addresses
which form the dispatcher takes and with which launch numbers (snvc_conv3d_forward_form, include/snvc_forms.h), and fails if the
row no longer reaches the form it is there for.  Then it runs the layer through snvc_amd.ops twice, requires equal bits, compares
with the float64 reference of the case module under test_gpu_parity.check (2e-5; 3e-4 for the k7 Winograd form) and requires the
buffer around a placed output to have kept its fill value.  A refused row must be refused by the query with the entry point's
status and text, and by the wrapper in its own way: an exception from Conv3dLayer, None from the three wrappers that have a
fallback.  Statistics rows compare the returned convolution; tests/test_gpu_stats_epilogue.py holds the moments.
"""
import functools
import os

import pytest
import torch

import conv_forward_cases as CC
import test_gpu_parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")) as _f:
    HEADER = _f.read()
LEAD = 64           # floats in front of a placed operand (256 bytes) and behind it


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8      # common.hpp device_cu_count()


@functools.lru_cache(maxsize=None)
def _values(name, cus):
    return CC.make_values(CC.BY_NAME[name], cus)


@functools.lru_cache(maxsize=None)
def _reference(name, cus):
    """(y, y_head) in float64, computed once per row and never written to."""
    y, y_head = CC.reference(CC.BY_NAME[name], _values(name, cus))
    out = y.numpy(), None if y_head is None else y_head.numpy()
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


class Placed:
    """A [N, ...] operand inside a buffer of FILL: 256 bytes + `off` behind a 256-byte boundary, batch stride padded by `pad`."""

    def __init__(self, shape, off=0, pad=0, value=None):
        assert off % 4 == 0
        n, per = shape[0], 1
        for s in shape[1:]:
            per *= s
        self.lo, self.bs, self.per, self.n = LEAD + off // 4, per + pad, per, n
        self.buf = torch.full((self.lo + n * self.bs + LEAD,), CC.FILL, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[self.lo:self.lo + n * self.bs].view(n, self.bs)[:, :per].view(shape)
        assert self.view.data_ptr() == self.buf.data_ptr() + 4 * self.lo
        if value is not None:
            self.view.copy_(value)

    def surroundings_kept(self):
        around = torch.ones_like(self.buf, dtype=torch.bool)
        around[self.lo:self.lo + self.n * self.bs].view(self.n, self.bs)[:, :self.per] = False
        return bool((self.buf[around] == CC.FILL).all())


def _layer(case, weight):
    from snvc_amd import ops
    k, s, dil, pad, transposed, planar, kh = CC.KEYS[case.key]
    return ops.Conv3dLayer(weight.to(DEV), k, s, pad, dil, transposed, planar=planar, ksize_h=kh)


def _ask(case, layer, cus, x, y, res, planes):
    """The dispatcher's decision for the call the wrapper is about to make: the descriptor `_desc` builds for it, the real addresses.
    What a wrapper allocates itself (the pooled or statistics output, a head's y_head) comes from torch's allocator, 256-byte
    aligned; `_run` checks that once it is back."""
    from snvc_amd import _forms, ops
    args = CC.desc_args(case, cus)
    assert args[4] == ops._batch_stride(x) and (y is None or args[5] == ops._batch_stride(y)) and (res is None or args[6] in (0, ops._batch_stride(res)))
    d = layer._desc(*args)
    al = lambda t: _forms.address_align(None if t is None else t.data_ptr())
    own = 16
    y_align = 0 if case.entry == "head" else al(y) if y is not None else own
    rc, info, text = _forms.conv3d_forward(d, CC.ENTRIES[case.entry], al(x), y_align, al(res), al(planes),
                                           own if case.entry in ("head", "side_head") else 0)
    assert (al(x), y_align, al(res), al(planes)) == CC.alignments(case)[:4], "the placement is not the row's"
    names = {v: k for k, v in _forms.enum_names(HEADER, "CF").items()}
    if case.form is None:
        assert rc == -case.refusal[0] and text.startswith(case.refusal[1]), (rc, text)
        return
    assert rc > 0 and names[rc] == case.form, f"{case.name}: the dispatcher takes {names.get(rc, rc)} ({text}), the row is there for {case.form}"
    assert info == CC.expected_numbers(case, cus), (case.name, info)


def _run(case, layer, x, y, res, planes, scale, bias, head_w):
    """One call through the wrapper of the row's entry point: (y, y_head), either None where the call has none; None when a
    wrapper with a fallback reports that the layer does not qualify."""
    from snvc_amd import ops
    own = lambda t: t if t.data_ptr() % 16 == 0 else pytest.fail("a wrapper's own output is not 16-byte aligned: the form was asked for another alignment")
    with torch.no_grad(), ops.conv_variant(case.bits):
        if case.entry == "stats":
            got = layer.forward_stats(x, torch.ones(case.cout, device=DEV), torch.zeros(case.cout, device=DEV), 1e-5)
            return None if got is None else (own(got[0]), None)
        if case.entry == "head":
            got = ops.conv3d_forward_head(layer, x, scale, bias, res, case.flags, head_w)
            return None if got is None else (None, own(got))
        if case.flags & CC.POOL:
            got = ops.conv3d_forward_avgpool_d4(layer, x, scale, bias, case.flags & ~CC.POOL)
            return None if got is None else (own(got), None)
        if case.entry == "side_head":
            out, y_head = layer(x, scale, bias, res, case.flags, out=y, side_head=head_w)
            return out, (None if y_head is None else own(y_head))
        return layer(x, scale, bias, res, case.flags, out=y, depth_planes=planes), None


@pytest.mark.parametrize("case", CC.GPU_CASES, ids=str)
def test_the_row_takes_its_form_and_matches_float64(case):
    from snvc_amd import _lib
    cus = _cus()
    v = _values(case.name, cus)
    layer = _layer(case, v["weight"])
    osp = CC.out_spatial(case.key, case.shape(cus))
    dev = lambda k: v[k].to(DEV) if k in v else None
    scale, bias, head_w = dev("scale"), dev("bias"), dev("head_w")
    x = Placed(tuple(v["x"].shape), case.off.get("x", 0), case.pad.get("x", 0), v["x"]).view
    res = Placed(tuple(v["residual"].shape), case.off.get("res", 0), case.pad.get("res", 0), v["residual"]).view if case.residual else None
    planes = Placed(tuple(v["planes"].shape), case.off.get("planes", 0), 0, v["planes"]).view if case.planes else None
    placed_out = case.entry in ("forward", "side_head") and not case.flags & CC.POOL
    outs = [Placed((case.n, case.cout) + osp, case.off.get("y", 0), case.pad.get("y", 0)) for _ in range(2)] if placed_out else [None, None]
    y0 = outs[0].view if placed_out else None

    _ask(case, layer, cus, x, y0, res, planes)

    if case.refusal is not None and placed_out and case.entry == "forward":
        with pytest.raises(_lib.Unsupported if case.refusal[0] == CC.UNSUPPORTED else RuntimeError) as e:
            _run(case, layer, x, y0, res, planes, scale, bias, head_w)
        assert case.refusal[1] in str(e.value)
        return
    first = _run(case, layer, x, y0, res, planes, scale, bias, head_w)
    if case.refusal is not None and case.entry != "side_head":
        assert first is None, "the wrapper ran a call the dispatcher refuses"
        return
    second = _run(case, layer, x, outs[1].view if placed_out else None, res, planes, scale, bias, head_w)
    torch.cuda.synchronize()
    if case.refusal is not None:        # a refused side head: the wrapper runs the layer alone and says so
        assert first[1] is None and second[1] is None
    tol = getattr(P, case.bound)
    ref_y, ref_head = _reference(case.name, cus)
    for got, again, ref, what in ((first[0], second[0], ref_y, "y"), (first[1], second[1], ref_head, "y_head")):
        if got is None:
            continue
        assert torch.equal(got, again), f"{case.name}: two runs differ in {what}"
        P.check(got.cpu().numpy(), ref, tol, f"{case.name} {what}")
    for o in outs:
        assert o is None or o.surroundings_kept(), f"{case.name}: the launch wrote outside its output"
