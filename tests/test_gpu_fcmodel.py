"""The FC box head on the GPU (snvc_amd.models.FCmodel, csrc/fc_head.hip) against the reference's recorded float64 results
(tests/golden/fcmodel_ref.npz) on the cases of tests/fcmodel_cases.py.

Tolerance.  The HIP routes and the reference's own float32 run differ from float64 only by summation order, ours also by one
rounding per weight from folding the norm.  The bound of a quantity is 8 (4 for the order times 2 for the fold) times the
largest error of the reference's float32 run for that quantity over the whole case table (`e32`, `train_e32` in the golden
file), relative to the quantity's own maximum: the table's maximum, because a single case's float32 error can be luckily small.
The yardstick comes from the reference, never from the kernels.  Each test prints its error beside the bound.
"""
import os
import types

import numpy as np
import pytest
import torch

import fcmodel_cases as FC
import fcmodel_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fcmodel_ref.npz"))
FACTOR = 8.0
EVAL_BOUND = FACTOR * np.max([GOLD[f"e32/{c.name}"] for c in FC.EVAL_CASES], axis=0)          # [output, representation]
TRAIN_BOUND = dict(zip(FC.TRAIN_KINDS, FACTOR * np.max([GOLD[f"train_e32/{c.name}"] for c in FC.TRAIN_CASES], axis=0)))


def dev():
    return torch.device("cuda:0")


def model_for(c, dtype=torch.float32):
    from snvc_amd.models.FCmodel import FCModel
    m = FCModel(**FC.ctor_kwargs(c))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in FC.state(c).items()}, strict=True)
    return m.to(dev(), dtype)


def routes():
    from snvc_amd.models import submodule as S
    return S._ROUTES["fc_hip"], S._ROUTES["fc_torch"]


def within(what, got, want, bound, scale=None):
    err = FC.rel_err(got.detach().cpu().numpy() if torch.is_tensor(got) else got, want, scale)
    print(f"{what}: error {err:.3g}, bound {bound:.3g}")
    assert np.shape(got) == np.shape(want) and err <= bound, f"{what}: {err:.3g} > {bound:.3g}"


# ---------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("c", FC.EVAL_CASES, ids=[c.name for c in FC.EVAL_CASES])
@pytest.mark.parametrize("hip", [True, False], ids=["hip", "torch"])
def test_eval_against_the_references_float64(c, hip):
    from snvc_amd.models import FCmodel
    m = model_for(c).eval()
    x = torch.from_numpy(FC.inputs(c)[0]).to(dev())
    h0, t0 = routes()
    FCmodel.FC_HIP[0] = hip
    try:
        with torch.no_grad():
            out, rep = m(x), m.get_representation(x)
    finally:
        FCmodel.FC_HIP[0] = True
    h1, t1 = routes()
    assert (h1 - h0, t1 - t0) == ((2, 0) if hip else (0, 2))
    assert out.dtype == torch.float32 and out.is_cuda
    within(f"{c.name} output", out, GOLD[f"out64/{c.name}"], EVAL_BOUND[0])
    within(f"{c.name} representation", rep, GOLD[f"rep64/{c.name}"], EVAL_BOUND[1])


def test_eval_does_not_touch_its_input_or_the_statistics():
    c = FC.BY_NAME["head_n17"]
    m = model_for(c).eval()
    x = torch.from_numpy(FC.inputs(c)[0]).to(dev())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        a, b = m(x), m(x)
    assert torch.equal(a, b) and torch.equal(x.cpu(), torch.from_numpy(FC.inputs(c)[0]))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


# ---------------------------------------------------------------------------------------------------- training
def train_step(c, m=None, masks="given"):
    """One step of sum(out * g) with the case's masks supplied through the hook -> (out, {name: grad}, state dict)."""
    m = model_for(c).train() if m is None else m
    x, g, case_masks = FC.inputs(c)
    if masks == "given" and case_masks is not None:
        on_dev = torch.from_numpy(case_masks).to(dev())
        m._draw_masks = lambda n, device: on_dev
    for p in m.parameters():
        p.grad = None
    x = torch.from_numpy(x).to(dev()).requires_grad_(True)
    out = m(x)
    (out * torch.from_numpy(g).to(dev())).sum().backward()
    grads = {"input": x.grad}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return out.detach(), grads, m.state_dict()


@pytest.mark.parametrize("c", FC.TRAIN_CASES, ids=[c.name for c in FC.TRAIN_CASES])
def test_training_step_against_the_references_float64(c):
    h0, t0 = routes()
    out, grads, sd = train_step(c)
    assert tuple(np.subtract(routes(), (h0, t0))) == (1, 0)
    pre = f"train64/{c.name}"
    within(f"{c.name} output", out, GOLD[f"{pre}/out"], TRAIN_BOUND["out"])
    within(f"{c.name} grad input", grads["input"], GOLD[f"{pre}/grad/input"], TRAIN_BOUND["grad_input"])
    assert len(grads) == 1 + 4 * (1 + 2 * c.blocks) + 2 and all(v is not None for v in grads.values())
    for k, v in grads.items():
        if k == "input":
            continue
        kind = FC.kind_of(k)
        scale = np.abs(GOLD[f"{pre}/grad/{k[:-4]}weight"]).max() if kind == "grad_zero_bias" else None
        within(f"{c.name} grad {k}", v, GOLD[f"{pre}/grad/{k}"], TRAIN_BOUND[kind], scale)
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(GOLD[f"{pre}/stat/{k}"]) == 4
        elif "running_" in k:
            within(f"{c.name} {k}", v, GOLD[f"{pre}/stat/{k}"], TRAIN_BOUND[FC.kind_of(k)])


def test_training_forward_without_gradients_is_the_same_forward():
    c = FC.BY_NAME["train_n17"]
    out, _, sd = train_step(c)
    m = model_for(c).train()
    on_dev = torch.from_numpy(FC.inputs(c)[2]).to(dev())
    m._draw_masks = lambda n, device: on_dev
    with torch.no_grad():
        again = m(torch.from_numpy(FC.inputs(c)[0]).to(dev()))
    assert torch.equal(out, again) and not again.requires_grad
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())      # the statistics moved the same way


def test_the_same_training_step_twice_gives_the_same_bits():
    c = FC.BY_NAME["train_w48"]
    out_a, grads_a, _ = train_step(c)
    out_b, grads_b, _ = train_step(c)
    assert torch.equal(out_a, out_b)
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def test_drawn_masks_follow_the_seed_and_keep_one_minus_p():
    c = FC.BY_NAME["train_n17"]
    m = model_for(c).train()
    drawn = []
    draw = m._draw_masks

    def recording(n, device):
        drawn.append(draw(n, device))
        return drawn[-1]
    m._draw_masks = recording
    torch.manual_seed(11)
    out_a, grads_a, _ = train_step(c, m, masks="drawn")
    torch.manual_seed(11)
    out_b, grads_b, _ = train_step(c, m, masks="drawn")
    assert torch.equal(drawn[0], drawn[1]) and torch.equal(out_a, out_b)
    assert all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    torch.manual_seed(12)
    assert not torch.equal(train_step(c, m, masks="drawn")[0], out_a)
    # the masks the module drew are the ones the kernels applied, each in its call slot
    sd, (x, _, _) = FC.state(c), FC.inputs(c)
    want, _ = R.forward(sd, x, c.blocks, c.leaky, train=True, masks=drawn[0].cpu().numpy(), p=c.p)
    within("output with drawn masks", out_a, want, TRAIN_BOUND["out"])
    # the kept fraction: a binomial bound of 6 sigma on 3 * 256 * 128 draws
    big = draw(256, dev())
    assert big.dtype == torch.uint8 and tuple(big.shape) == (3, 256, 128) and int(big.max()) == 1
    count = big.numel()
    kept = float(big.float().mean())
    sigma = (c.p * (1 - c.p) / count) ** 0.5
    print(f"kept fraction {kept:.4f}, 1 - p = {1 - c.p}, 6 sigma = {6 * sigma:.4f}")
    assert abs(kept - (1 - c.p)) <= 6 * sigma
    # p = 0: no masks at all
    assert model_for(FC.BY_NAME["train_n2"])._draw_masks(4, dev()) is None


def test_one_row_in_train_mode_raises_as_torch_does():
    c = FC.BY_NAME["head_n1"]
    m = model_for(c).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(torch.from_numpy(FC.inputs(c)[0]).to(dev()))


# ---------------------------------------------------------------------------------------------------- the packed buffer
def test_packed_buffer_follows_the_parameters():
    a, b = FC.BY_NAME["head_n17"], FC.BY_NAME["head_n1"]
    m = model_for(a).eval()
    xa, xb = (torch.from_numpy(FC.inputs(c)[0]).to(dev()) for c in (a, b))
    with torch.no_grad():
        within("before", m(xa), GOLD[f"out64/{a.name}"], EVAL_BOUND[0])
        packed = m._packed(dev())
        assert m._packed(dev()) is packed                                       # built once
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in FC.state(b).items()}, strict=True)
        within("after load_state_dict", m(xb), GOLD[f"out64/{b.name}"], EVAL_BOUND[0])
        assert m._packed(dev()) is not packed
        m.res_blocks[0].batch_norm2.running_var.mul_(1.7)                       # in place, as a training step's update is
        sd = FC.state(b)
        sd["res_blocks.0.batch_norm2.running_var"] = sd["res_blocks.0.batch_norm2.running_var"] * np.float32(1.7)
        want, _ = R.forward(sd, FC.inputs(b)[0], b.blocks, b.leaky)
        assert FC.rel_err(want, GOLD[f"out64/{b.name}"]) > 100 * EVAL_BOUND[0]  # the change is far above the bound
        within("after an in-place running_var change", m(xb), want, EVAL_BOUND[0])


def test_a_training_step_is_seen_by_the_next_eval_call():
    c = FC.BY_NAME["train_n17"]
    m = model_for(c).eval()
    x = torch.from_numpy(FC.inputs(c)[0]).to(dev())
    with torch.no_grad():
        m(x)
    _, _, sd = train_step(c, m.train())
    m.eval()
    with torch.no_grad():
        got = m(x)
    want, _ = R.forward({k: v.cpu().numpy() for k, v in sd.items()}, FC.inputs(c)[0], c.blocks, c.leaky)
    within("eval after a training step", got, want, EVAL_BOUND[0])


# ---------------------------------------------------------------------------------------------------- routes
def test_routes():
    from snvc_amd.models.FCmodel import FCModel
    c = FC.BY_NAME["head_n17"]
    x = torch.from_numpy(FC.inputs(c)[0]).to(dev())
    h0, t0 = routes()
    with torch.no_grad():
        out64 = model_for(c, torch.float64).eval()(x.double())                      # float64: the modules' torch forward
    assert tuple(np.subtract(routes(), (h0, t0))) == (0, 1) and out64.dtype == torch.float64
    assert FC.rel_err(out64.cpu().numpy(), GOLD[f"out64/{c.name}"]) < 1e-12
    torch.manual_seed(3)
    narrow = FCModel(num_neurons=40, num_blocks=1, input_size=18, output_size=5).to(dev()).eval()      # 40 is no multiple of 16
    with torch.no_grad():
        got = narrow(x)
    assert tuple(np.subtract(routes(), (h0, t0))) == (0, 2)
    want, _ = R.forward({k: v.cpu().numpy() for k, v in narrow.state_dict().items()}, FC.inputs(c)[0], 1)
    assert FC.rel_err(got.cpu().numpy(), want) < 1e-5
    m = model_for(c).eval()
    m(x)                                                                              # eval-mode norms under autograd: torch
    assert tuple(np.subtract(routes(), (h0, t0))) == (0, 3)
    m.res_blocks[0].batch_norm1.train()                                               # a mix of modes: torch
    with torch.no_grad():
        m(x)
    assert tuple(np.subtract(routes(), (h0, t0))) == (0, 4)
    m = model_for(c).eval()          # a fresh one: the train-mode norm above moved its running statistics
    with torch.no_grad():
        m(x)                                                                          # eligible
        assert tuple(np.subtract(routes(), (h0, t0))) == (1, 4)
        strided = torch.from_numpy(np.repeat(FC.inputs(c)[0], 2, axis=1)).to(dev())[:, ::2]
        assert not strided.is_contiguous()
        got = m(strided)                                                              # a strided view: torch
    assert tuple(np.subtract(routes(), (h0, t0))) == (1, 5)
    within("strided input on the torch route", got, GOLD[f"out64/{c.name}"], EVAL_BOUND[0])


# ---------------------------------------------------------------------------------------------------- VernierScale
def vernier_with_head():
    import golden_cases as GC
    from oracle import torch_ref as T
    from snvc_amd.models.vernier import VernierScale
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES["G1"]
    m = VernierScale(FC.vernier_cfg(grid, use_bbox_head=True))
    m.load_state_dict(T.seeded_state_dict(m, seed), strict=True)
    inputs = [t.to(dev()) for t in GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)]
    return m.to(dev()), inputs, n


def test_vernier_scale_returns_the_box():
    m, inputs, n = vernier_with_head()
    m.eval()
    h0, t0 = routes()
    with torch.no_grad():
        out = m(*inputs)
        assert tuple(np.subtract(routes(), (h0, t0))) == (1, 0)
        want = m.bbox_head(out["coordinates"].reshape(n, -1))
    assert set(out) == {"ncf", "occupancy", "coordinates", "bbox"}
    assert tuple(out["bbox"].shape) == (n, 5) and torch.equal(out["bbox"], want)
    # and the head is the FC model of the case table: the same module on the same numbers, against the restatement
    ref, _ = R.forward({k: v.cpu().numpy() for k, v in m.bbox_head.state_dict().items()},
                       out["coordinates"].reshape(n, -1).cpu().numpy(), 1)
    within("bbox", out["bbox"], ref, EVAL_BOUND[0])


def test_bbox_loss_trains_the_coordinate_head_through_the_box_head():
    from snvc_amd.models.loss3d import BboxLoss
    m, inputs, n = vernier_with_head()
    m.train()
    h0, t0 = routes()
    out = m(*inputs)
    assert tuple(np.subtract(routes(), (h0, t0))) == (1, 0) and out["bbox"].requires_grad
    gt = torch.from_numpy(np.random.default_rng(5).standard_normal((n, 5)).astype(np.float32))
    loss = BboxLoss(types.SimpleNamespace(head_reg_type="2D"))(out, {"gt_box_local": gt})["l1"]
    loss.backward()
    head = [p.grad for p in m.coord_head.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in head) and any(float(g.abs().max()) > 0 for g in head)
    assert all(p.grad is not None for p in m.bbox_head.parameters())
