"""The device read-out (snvc_amd.decode.refine_boxes, csrc/decode.hip) and snvc_amd.refine.Refiner on the GPU.

Two references.  The reference's own outputs (tests/golden/decode_outputs.npz) for the three inputs of
tests/test_decode.py::decode_case: flags and confidences equal, boxes within 1e-9, the tolerance tests/test_decode.py gives the
host route against the same file.  And the host route (decode.ncf_to_update_2d on the numpy copy of the same inputs, pinned
to that file) for the cases of tests/decode_cases.py, whose conditions tests/test_decode_device_host.py asserts: indices,
confidences and flags equal, boxes within 1e-9.  The float32 `coordinates` are handed to the host route widened to float64,
which is what the kernel does with them (numpy would otherwise apply the range in float32).

Largest |device - host| over every box, measured on the MI355X: 3.55e-14 (case "edges"; the reference's fixtures 2.13e-14,
the Refiner's end-to-end case 1.02e-14), against the 1e-9 allowed.
"""
import copy
import types

import numpy as np
import pytest
import torch

import decode_cases as C
import golden_cases as GC
import roi_crop_cases as RC
from benchlib import hrnet as B
from benchlib.common import seeded_state
from test_decode import GOLDEN, decode_case
from snvc_amd import decode as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-9
KEYS = ("all_parts", "one_part", "confidence", "index", "keep_flags")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_of(res):
    return {k: (None if res[k] is None else res[k].cpu().numpy()) for k in KEYS}


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def host_route(c, ncf=None, filter_3d=None):
    co = None if c["coordinates"] is None else c["coordinates"].astype(np.float64)
    return D.ncf_to_update_2d(c["cfg"], c["ncf"] if ncf is None else ncf, c["samples"].copy(), c["grid"], filter_3d or D.Filter(), coordinates=co)


def check_against_host(name, got, c, host):
    """Shapes, dtypes, the exact parts and the boxes; returns the largest box difference."""
    ncf = c["ncf"]
    n, parts = ncf.shape[:2]
    assert got["confidence"].dtype == np.float32 and got["confidence"].shape == (n, parts)
    assert got["index"].dtype == np.int64 and got["index"].shape == (n, parts)
    assert got["keep_flags"].dtype == np.bool_ and got["keep_flags"].shape == (n,)
    assert got["one_part"].dtype == np.float64 and got["one_part"].shape == (n, 7)
    keep = host["keep_flags"]
    assert np.array_equal(got["keep_flags"], keep)
    assert np.array_equal(got["confidence"], host["confidence"], equal_nan=True)
    assert np.array_equal(got["index"], ncf.reshape(n, parts, -1).argmax(axis=2))
    assert np.array_equal(got["one_part"][~keep], c["samples"][~keep])
    worst = 0.0
    if parts > 1:
        assert got["all_parts"].dtype == np.float64 and got["all_parts"].shape == (n, 7)
        assert np.array_equal(got["all_parts"][~keep], c["samples"][~keep])
        worst = np.abs(got["all_parts"] - np.asarray(host["pred"]["all_parts"])).max()
        one = got["one_part"][keep]
    else:
        assert got["all_parts"] is None
        one = got["one_part"]
    if len(one):
        worst = max(worst, np.abs(one - np.asarray(host["pred"]["one_part"])).max())
    print(f"{name}: largest |device - host| over the boxes {worst:.3g}")
    assert worst <= ATOL
    return worst


# ---------------------------------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("name", ["argmax", "coordinates", "one_part_only"])
def test_reference_fixtures(name):
    G = np.load(GOLDEN)
    c = decode_case(name)
    got = host_of(D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"].copy(), c["grid"].copy(), coordinates=c["coordinates"]))
    keep = G[f"{name}/keep_flags"]
    assert np.array_equal(got["keep_flags"], keep) and keep.sum() == 4
    assert np.array_equal(got["confidence"], G[f"{name}/confidence"])
    if name == "one_part_only":
        assert got["all_parts"] is None
        np.testing.assert_allclose(got["one_part"], G[f"{name}/pred_one_part"], rtol=0, atol=ATOL)
    else:
        np.testing.assert_allclose(got["all_parts"], G[f"{name}/pred_all_parts"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(got["one_part"][keep], G[f"{name}/pred_one_part"], rtol=0, atol=ATOL)
    check_against_host(name, got, c, host_route(c))


# ---------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", C.NAMES)
def test_cases_equal_the_host_route(name):
    c = C.case(name)
    co = c["coordinates"]
    if name == "coords_f32":
        co = dev(co)                                 # a float32 device tensor; the others stay float64 numpy
    got = host_of(D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"], c["grid"], coordinates=co))
    check_against_host(name, got, c, host_route(c))
    assert np.array_equal(got["keep_flags"], c["expect_keep"])
    if name == "m1247_ties":
        for (i, p), (lo, _) in C.TIES.items():
            assert got["index"][i, p] == lo and got["confidence"][i, p] == C.TIE_VALUE
    if name == "edges":
        i, p, cells = C.NAN_AT
        assert got["index"][i, p] == cells[0] and np.isnan(got["confidence"][i, p]) and not got["keep_flags"][i]
        assert np.array_equal(got["one_part"][i], c["samples"][i]) and np.array_equal(got["all_parts"][i], c["samples"][i])
        assert got["index"][6, 5] == 0 and got["confidence"][6, 5] == 0.0 and got["keep_flags"][6]
    if name == "m1_coords":
        assert not got["index"].any()


def test_no_instances():
    c = C.case("m35")
    for parts in (9, 1):
        res = D.refine_boxes(c["cfg"], dev(c["ncf"][:0, :parts]), c["samples"][:0], c["grid"])
        torch.cuda.synchronize()
        assert res["one_part"].shape == (0, 7) and res["one_part"].dtype == torch.float64
        assert res["confidence"].shape == (0, parts) and res["confidence"].dtype == torch.float32
        assert res["index"].shape == (0, parts) and res["index"].dtype == torch.int64
        assert res["keep_flags"].shape == (0,) and res["keep_flags"].dtype == torch.bool
        if parts == 9:
            assert res["all_parts"].shape == (0, 7) and res["all_parts"].dtype == torch.float64
        else:
            assert res["all_parts"] is None
        assert all(v is None or v.is_cuda for v in res.values())
        assert D.to_update_dict(res)["pred"]["one_part"] == []


def test_views_and_other_dtypes_go_through_float_contiguous():
    c = C.case("m35")
    plain = host_of(D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"], c["grid"]))
    view = dev(c["ncf"].transpose(0, 1, 3, 2)).permute(0, 1, 3, 2)
    assert not view.is_contiguous() and torch.equal(view, dev(c["ncf"]))
    assert same_bits(host_of(D.refine_boxes(c["cfg"], view, c["samples"], c["grid"])), plain)
    half = dev(c["ncf"]).half()
    got = host_of(D.refine_boxes(c["cfg"], half, c["samples"], c["grid"]))
    rounded = half.float().cpu().numpy()
    check_against_host("m35 as float16", got, dict(c, ncf=rounded), host_route(c, ncf=rounded))
    double = host_of(D.refine_boxes(c["cfg"], dev(c["ncf"]).double(), c["samples"], c["grid"]))
    assert same_bits(double, plain)


def test_device_inputs_equal_numpy_inputs_and_are_left_alone():
    for name in ("m35", "coords_f64"):
        c = C.case(name)
        ncf, samples, grid = dev(c["ncf"]), dev(c["samples"]), dev(c["grid"])
        co = None if c["coordinates"] is None else dev(c["coordinates"])
        version, before = ncf._version, samples.clone()
        on_device = D.refine_boxes(c["cfg"], ncf, samples, grid, coordinates=co)
        assert ncf._version == version and samples._version == before._version and torch.equal(samples, before)
        assert on_device["one_part"].data_ptr() != samples.data_ptr() and on_device["all_parts"].data_ptr() != samples.data_ptr()
        from_numpy = D.refine_boxes(c["cfg"], ncf, c["samples"], c["grid"], coordinates=c["coordinates"])
        assert same_bits(host_of(on_device), host_of(from_numpy))


def test_a_wide_filter_and_the_update_dict():
    c = C.case("edges")
    wide = D.Filter(-1e30, 1e30)
    res = D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"], c["grid"], filter_3d=wide)
    host = host_route(c, filter_3d=wide)
    assert host["keep_flags"].tolist() == [True, True, True, False, False, False, True]       # +-inf and NaN stay out
    check_against_host("edges, wide filter", host_of(res), c, host)
    got = D.to_update_dict(res)
    assert np.array_equal(got["keep_flags"], host["keep_flags"]) and np.array_equal(got["confidence"], host["confidence"], equal_nan=True)
    for k in ("one_part", "all_parts"):
        assert len(got["pred"][k]) == len(host["pred"][k])
        np.testing.assert_allclose(np.asarray(got["pred"][k]), np.asarray(host["pred"][k]), rtol=0, atol=ATOL)


def test_refusals():
    c = C.case("m35")
    with pytest.raises(TypeError, match="Filter"):
        D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"], c["grid"], filter_3d=object())
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        D.refine_boxes(c["cfg"], torch.from_numpy(c["ncf"]), c["samples"], c["grid"])
    with pytest.raises(ValueError, match="1 or 9"):
        D.refine_boxes(c["cfg"], dev(c["ncf"][:, :5]), c["samples"], c["grid"])
    with pytest.raises(ValueError, match="grid"):
        D.refine_boxes(c["cfg"], dev(c["ncf"]), c["samples"], c["grid"][:-1])


# ---------------------------------------------------------------------------------------------------- Refiner
def _e2e_cfg():
    """tests/test_gpu_hrnet.py::_e2e_cfg, with the y_range GridProjector and grid_bev_flat read."""
    grid = (16, 16, 24)
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=False, grid_resolution=list(grid),
                                resolution=GC.RESOLUTION, x_range=(-1.0, 1.0), y_range=(-0.8, 0.8), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = copy.deepcopy(B.E2E_HRNET)
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    return cfg


@pytest.fixture(scope="module")
def e2e():
    from snvc_amd.models.vernier import VernierScale
    cfg = _e2e_cfg()
    m = VernierScale(cfg)
    m.load_state_dict(seeded_state(m, B.E2E_SEEDS[0]), strict=True)
    m.to(DEV).eval()
    rc = RC.case("gradient_64")
    assert rc["cfg"].resolution == tuple(cfg.resolution)
    # one pass before anything is compared: the seeded features (~300) overflow split mode in the trunk, the model redoes
    # that call in fp32 and stays on the fp32 kernels from then on (split_mode.py), so that every later call takes one route
    from snvc_amd.refine import Refiner
    Refiner(m, rc["cfg"]).refine(rc["samples"], rc["left"][0], rc["right"][0], rc["P_left"][0], rc["P_right"][0])
    return m, cfg, rc


@pytest.mark.parametrize("which", ["default", "wide"])
def test_refiner_equals_the_four_steps_by_hand(e2e, which):
    """The seeded model's maps lie in about [-4000, 4200], so the default Filter's [-1, 2] rejects all four instances (every
    output is then the proposal); the same comparison is made under Filter(-1e30, 1e30), which keeps all four."""
    from snvc_amd.geometry import GridProjector, RoICropper
    from snvc_amd.refine import Refiner
    m, cfg, rc = e2e
    filt = None if which == "default" else D.Filter(-1e30, 1e30)
    args = (rc["samples"], rc["left"][0], rc["right"][0], rc["P_left"][0], rc["P_right"][0])
    before = set(m.__dict__)
    got = Refiner(m, rc["cfg"], filter_3d=filt).refine(*args)
    assert not {k for k in set(m.__dict__) - before if not k.startswith("_snvc_")}      # the model's own plan caches may appear
    left, right, meta = RoICropper(rc["cfg"]).generate(*args, DEV)
    coord_l, coord_r = GridProjector(cfg).generate(rc["samples"], rc["P_left"][0], rc["P_right"][0], meta["trans_l"], meta["trans_r"], DEV)
    with torch.no_grad():
        out = m(left, right, coord_l, coord_r)
    version = out["ncf"]._version
    assert same_bits(host_of(m.refine_boxes(out["ncf"], rc["samples"], D.grid_bev_flat(cfg), filt, coordinates=out["coordinates"])), host_of(got))
    assert out["ncf"]._version == version
    ncf = out["ncf"].cpu().numpy()
    print(f"{which}: the model's maps lie in [{ncf.min():.3g}, {ncf.max():.3g}]")
    c = dict(cfg=cfg, ncf=ncf, samples=rc["samples"], grid=D.grid_bev_flat(cfg), coordinates=out["coordinates"].cpu().numpy())
    host = host_route(c, filter_3d=filt)
    if which == "wide":
        assert host["keep_flags"].all()
    boxes = np.asarray(host["pred"]["all_parts"])
    assert (np.abs(boxes[host["keep_flags"], 6]) <= np.pi - 1e-6).all()
    check_against_host(f"refiner, {which} filter ({int(host['keep_flags'].sum())} of {len(boxes)} kept)", host_of(got), c, host)


def test_refiner_iterations_chain_on_the_device(e2e):
    from snvc_amd.refine import Refiner
    m, cfg, rc = e2e
    refiner = Refiner(m, rc["cfg"], filter_3d=D.Filter(-1e30, 1e30))
    samples = dev(rc["samples"])
    rest = (rc["left"][0], rc["right"][0], rc["P_left"][0], rc["P_right"][0])
    kept = samples.clone()
    twice = refiner.refine(samples, *rest, iterations=2)
    assert torch.equal(samples, kept)
    first = refiner.refine(samples, *rest)
    second = refiner.refine(first["all_parts"], *rest)
    assert first["all_parts"].is_cuda and not torch.equal(first["all_parts"], samples)
    want = host_of(second)
    want["keep_flags"] = want["keep_flags"] & first["keep_flags"].cpu().numpy()
    assert same_bits(host_of(twice), want)
    # a rejected instance stays rejected in the AND, whatever the second pass says of its unchanged proposal
    strict = Refiner(m, rc["cfg"], filter_3d=D.Filter(1e30, -1e30)).refine(samples, *rest, iterations=2)
    assert not strict["keep_flags"].any() and torch.equal(strict["all_parts"], samples) and torch.equal(strict["one_part"], samples)
