"""CPU checks of the FC box head's host side: the module tree of snvc_amd.models.FCmodel against the reference's recorded
state-dict keys, the float64 restatement (tests/fcmodel_ref.py) against the reference's recorded float64 results
(tests/golden/fcmodel_ref.npz, written by tests/golden/make_golden_fcmodel.py) and against torch's autograd, the binding
against include/snvc_fc.h, the alias, and VernierScale's construction with and without the head.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fcmodel_cases as FC
import fcmodel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_fc.h")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fcmodel_ref.npz"))


# ---------------------------------------------------------------------------------------------------- the module tree
@pytest.mark.parametrize("tag", ["head", "defaults"])
def test_state_dict_keys_order_and_shapes_are_the_references(tag):
    from snvc_amd.models.FCmodel import FCModel, get_fc_model
    sd = (get_fc_model() if tag == "head" else FCModel()).state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[f"keys/{tag}"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in GOLD[f"shapes/{tag}"]]


def test_case_table_names_the_modules_keys():
    from snvc_amd.models.FCmodel import FCModel
    for c in FC.EVAL_CASES + FC.TRAIN_CASES:
        m = FCModel(**FC.ctor_kwargs(c))
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == FC.state_keys(c)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in FC.state(c).items()}, strict=True)


def test_constructor_arguments_and_the_kaiming_quirk():
    from snvc_amd.models.FCmodel import FCModel, ResidualBlock, get_fc_model
    m = get_fc_model()
    assert (m.num_neurons, m.num_blocks, m.input_size, m.output_size, m.p_dropout, m.leaky) == (128, 1, 18, 5, 0.5, False)
    d = FCModel()
    assert (d.num_neurons, d.num_blocks, d.input_size, d.output_size, d.p_dropout, d.leaky) == (1024, 2, 32, 64, 0.5, False)
    assert isinstance(FCModel(num_neurons=16, num_blocks=1, leaky=True).res_blocks[0].relu, torch.nn.LeakyReLU)
    # kaiming reaches the model's own two Linears and not its blocks': a block's weights keep nn.Linear's bound 1 / sqrt(fan_in)
    torch.manual_seed(0)
    k = FCModel(num_neurons=256, num_blocks=1, kaiming=True, input_size=256)
    assert float(k.w1.weight.detach().abs().max()) > 1.0 / 16 and float(k.res_blocks[0].w1.weight.detach().abs().max()) <= 1.0 / 16
    assert float(ResidualBlock(256, kaiming=True).w1.weight.detach().abs().max()) > 1.0 / 16


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("c", FC.EVAL_CASES, ids=[c.name for c in FC.EVAL_CASES])
def test_restatement_eval_equals_the_reference(c):
    sd, (x, _, _) = FC.state(c), FC.inputs(c)
    out, _ = R.forward(sd, x, c.blocks, c.leaky)
    rep, _ = R.forward(sd, x, c.blocks, c.leaky, representation=True)
    assert out.shape == (c.n, c.output) and rep.shape == (c.n, c.neurons)
    assert np.abs(out - GOLD[f"out64/{c.name}"]).max() <= 1e-12 * max(1.0, np.abs(out).max())
    assert np.abs(rep - GOLD[f"rep64/{c.name}"]).max() <= 1e-12 * max(1.0, np.abs(rep).max())


def restated_step(c):
    sd, (x, g, masks) = FC.state(c), FC.inputs(c)
    out, cache = R.forward(sd, x, c.blocks, c.leaky, train=True, masks=masks, p=c.p)
    dx, grads = R.backward(cache, g)
    return sd, out, dx, grads, R.updated_stats(sd, cache)


@pytest.mark.parametrize("c", FC.TRAIN_CASES, ids=[c.name for c in FC.TRAIN_CASES])
def test_restatement_train_equals_the_reference(c):
    _, out, dx, grads, stats = restated_step(c)
    pre = f"train64/{c.name}"

    def close(got, want):
        # the batch of two is ill-conditioned (a neuron's two values can lie 1e-3 apart under eps = 1e-5): float64 runs that
        # sum in another order differ by 1e-16 times the conditioning there, far below 1e-12 either way
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    close(out, GOLD[f"{pre}/out"])
    close(dx, GOLD[f"{pre}/grad/input"])
    names = [k[len(pre) + 6:] for k in GOLD.files if k.startswith(f"{pre}/grad/") and not k.endswith("/input")]
    assert sorted(names) == sorted(grads) and len(names) == 4 * (1 + 2 * c.blocks) + 2
    for k in names:
        close(grads[k], GOLD[f"{pre}/grad/{k}"])
    for k, v in stats.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(GOLD[f"{pre}/stat/{k}"]) == 4
        else:
            close(v, GOLD[f"{pre}/stat/{k}"])


@pytest.mark.parametrize("c", FC.TRAIN_CASES, ids=[c.name for c in FC.TRAIN_CASES])
def test_restatement_gradients_equal_torch_autograd(c):
    sd, _, dx, grads, _ = restated_step(c)
    x, g, masks = FC.inputs(c)
    t = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in sd.items() if v.dtype != np.int64}
    xt = torch.from_numpy(x).double().requires_grad_(True)
    cur, block_in = xt, None
    for i, (lin, bn) in enumerate(FC.layer_prefixes(c.blocks)):
        if i % 2 == 1:
            block_in = cur
        y = F.batch_norm(F.linear(cur, t[f"{lin}.weight"], t[f"{lin}.bias"]), None, None, t[f"{bn}.weight"], t[f"{bn}.bias"], True)
        y = F.leaky_relu(y, 0.01) if c.leaky else F.relu(y)
        if masks is not None:
            y = y * torch.from_numpy(masks[i]).double() / (1.0 - c.p)
        cur = y + block_in if (i > 0 and i % 2 == 0) else y
    out = F.linear(cur, t["w2.weight"], t["w2.bias"])
    (out * torch.from_numpy(g).double()).sum().backward()
    assert np.abs(dx - xt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dx).max())
    for k, v in grads.items():
        assert np.abs(v - t[k].grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(v).max()), k


# ---------------------------------------------------------------------------------------------------- binding, alias, model
def test_header_and_binding_agree():
    """The mirrored constant and the packed size; names, parameters and the ABI number are held by
    tests/test_abi_tables_host.py."""
    from snvc_amd import _fc
    text = open(HEADER).read()
    assert int(re.search(r"SNVC_FC_MAX_WIDTH = (\d+)", text).group(1)) == _fc.MAX_WIDTH
    L = _fc.lib()
    assert L.snvc_fc_packed_floats(18, 128, 1, 5) == 20 * 128 + 128 + 2 * (128 * 128 + 128) + 128 * 16 + 16
    assert L.snvc_fc_packed_floats(18, 40, 1, 5) < 0 and L.snvc_fc_packed_floats(18, 2048, 1, 5) < 0


def test_the_c_calls_check_their_arguments_before_any_launch():
    from snvc_amd import _fc
    from snvc_amd._lib import lib
    L = _fc.lib()
    assert L.snvc_fc_eval_forward(None, None, None, 0, 18, 128, 1, 5, 0, 0, None) == 0          # N = 0: nothing to do
    assert L.snvc_fc_eval_forward(None, None, None, 4, 18, 128, 1, 5, 0, 0, None) == 1 and b"null pointer" in lib().snvc_last_error_string()
    assert L.snvc_fc_eval_forward(None, None, None, 4, 18, 40, 1, 5, 0, 0, None) == 1 and b"multiple of 16" in lib().snvc_last_error_string()
    one = 16        # a non-null, aligned stand-in: the size checks come before any pointer is read
    assert L.snvc_fc_train_layer_forward(*([one] * 14), 1, 18, 128, 1e-5, 0.1, 1.0, 0, None) == 1
    assert b"more than one row" in lib().snvc_last_error_string()
    assert L.snvc_fc_train_layer_forward(*([one] * 14), 4, 18, 40, 1e-5, 0.1, 1.0, 0, None) == 1
    assert L.snvc_fc_train_layer_backward_params(*([None] * 12), 4, 18, 128, 1.0, 0, None) == 1
    assert L.snvc_fc_train_layer_backward_input(None, None, None, None, 4, 2000, 128, None) == 1


def test_install_as_snvc_aliases_the_module():
    import snvc_amd
    saved = {k: sys.modules.get(k) for k in list(snvc_amd._ALIASES) + ["snvc", "snvc.models", "snvc.extension"]}
    try:
        snvc_amd.install_as_snvc(backbone=False)
        from snvc.models.FCmodel import get_fc_model
        from snvc_amd.models import FCmodel
        assert get_fc_model is FCmodel.get_fc_model and sys.modules["snvc.models.FCmodel"] is FCmodel
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_vernier_scale_constructs_with_the_box_head():
    from snvc_amd.models.FCmodel import FCModel
    from snvc_amd.models.vernier import VernierScale
    plain = VernierScale(FC.vernier_cfg())
    with_head = VernierScale(FC.vernier_cfg(use_bbox_head=True))
    assert isinstance(with_head.bbox_head, FCModel) and not hasattr(plain, "bbox_head")
    head_keys = [k for k in with_head.state_dict() if k.startswith("bbox_head.")]
    assert head_keys == ["bbox_head." + str(k) for k in GOLD["keys/head"]]
    assert [k for k in with_head.state_dict() if not k.startswith("bbox_head.")] == list(plain.state_dict())
    # the head belongs to BEV_type3 only, as in the reference
    assert not hasattr(VernierScale(FC.vernier_cfg((32, 32, 48), vernier_type="BEV_type2", use_bbox_head=True)), "bbox_head")


def test_a_cpu_input_raises():
    from snvc_amd.models.FCmodel import get_fc_model
    m = get_fc_model().eval()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m(torch.zeros(2, 18))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m.get_representation(torch.zeros(2, 18))
