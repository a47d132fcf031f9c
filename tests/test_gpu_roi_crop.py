"""snvc_amd.geometry.RoICropper on the GPU against the numpy restatement of its specification (tests/roi_crop_ref.py; the
cases and the margins that make their decisions safe: tests/roi_crop_cases.py, asserted by tests/test_roi_crop_host.py).

Tolerances.  Raw crops are integers decided with a margin (every value handed to R(.) is 1e-6 from a half-integer, every
'exact' coordinate 1e-6 from an integer, while the device's float64 geometry differs from numpy's by about 1e-13): bit-equal.
Normalised crops are a table lookup of torch's own CPU results: torch.equal.  trans and kpts_2d: 1e-10 absolute (fma chains
and the device's sin / cos against numpy's matmul and libm).  kpts_2d_local is float32(trans . [kpts; 1]) of float64 values
that differ by that noise, so the cast may land on the neighbouring float32 where the value sits at a rounding boundary: it
is held to 1 ulp of float32, not to equality.  (The points lie inside the crop, at least 4.5 % of a side from its edge, so
none is near zero, where an absolute noise would be many ulps.)
"""
import functools

import numpy as np
import pytest
import torch

import roi_crop_cases as C
import roi_crop_ref as R
from snvc_amd.geometry import GridProjector, RoICropper

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMETRY_TOL = 1e-10
MODES = ("fixed5", "exact")
ORDERS = ("rgb", "bgr")


@functools.lru_cache(maxsize=None)
def expected(name, mode, order):
    """The restatement's answer, computed once and shared: raw uint8 [2][N,3,Hr,Wr], kpts, trans, local per side."""
    c = C.case(name)
    out = {k: ([], []) for k in ("raw", "kpts", "trans", "local")}
    for n, s in enumerate(c["samples"]):
        f = C.frame_of(c, n)
        for side, (imgs, P) in enumerate(((c["left"], c["P_left"]), (c["right"], c["P_right"]))):
            for key, val in zip(("raw", "kpts", "trans", "local"), R.crop(s, imgs[f], P[f], c["cfg"], mode, order)):
                out[key][side].append(val)
    return {k: tuple(np.stack(v) for v in pair) for k, pair in out.items()}


def run(name, mode="fixed5", order="rgb", raw=True, use_frame=None, **kw):
    c = C.case(name)
    single = c["frame"] is None
    frame = c["frame"] if not single else (np.zeros(len(c["samples"]), dtype=np.int64) if use_frame else None)
    left, right = (c["left"][0], c["right"][0]) if single and not use_frame else (c["left"], c["right"])
    P_l, P_r = (c["P_left"][0], c["P_right"][0]) if single else (c["P_left"], c["P_right"])
    out = RoICropper(c["cfg"]).generate(c["samples"], left, right, P_l, P_r, DEV, frame=frame, raw=raw, interpolation=mode,
                                        channel_order=order, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", C.NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
def test_raw_crops_are_bit_equal(name, mode, order):
    want = expected(name, mode, order)["raw"]
    for use_frame in (False, True):
        left, right, _ = run(name, mode, order, use_frame=use_frame)
        for side, got in enumerate((left, right)):
            got = got.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == want[side].shape
            bad = int((got != want[side]).sum())
            print(f"{name} {mode} {order} frame={use_frame} side {side}: {bad} of {got.size} bytes differ")
            assert bad == 0


@pytest.mark.parametrize("name", C.NAMES)
def test_normalised_crops_equal_torch_cpu(name):
    c = C.case(name)
    want = expected(name, "fixed5", "rgb")["raw"]
    left, right, _ = run(name, raw=False)
    for side, got in enumerate((left, right)):
        ref = torch.stack([R.normalise(crop.transpose(1, 2, 0), c["cfg"].img_mean, c["cfg"].img_std) for crop in want[side]])
        assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_contiguous()
        assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("name", C.NAMES)
def test_geometry_matches_the_restatement(name):
    want = expected(name, "fixed5", "rgb")
    _, _, meta = run(name)
    for side, s in enumerate("lr"):
        trans, kpts, local = (meta[k].cpu().numpy() for k in (f"trans_{s}", f"kpts_2d_{s}", f"kpts_2d_{s}_local"))
        assert trans.dtype == np.float64 and kpts.dtype == np.float64 and local.dtype == np.float32
        assert trans.shape == want["trans"][side].shape and kpts.shape == want["kpts"][side].shape and local.shape == want["local"][side].shape
        dt, dk = np.abs(trans - want["trans"][side]).max(), np.abs(kpts - want["kpts"][side]).max()
        ulp = (np.abs(local - want["local"][side]) / np.spacing(np.abs(want["local"][side]))).max()
        print(f"{name} side {s}: max |trans - ref| {dt:.3g}, |kpts - ref| {dk:.3g}, local {ulp:.3g} ulp, "
              f"{int((local != want['local'][side]).sum())} of {local.size} local values differ")
        assert dt <= GEOMETRY_TOL and dk <= GEOMETRY_TOL
        assert ulp <= 1.0
        assert (trans[:, 0, 1] == 0).all() and (trans[:, 1, 0] == 0).all()


def test_same_input_same_bits_and_a_side_stream():
    first = run("two_frames", raw=False)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        second = run("two_frames", raw=False)
    stream.synchronize()
    for a, b in zip(first[:2], second[:2]):
        assert torch.equal(a, b)
    for k in first[2]:
        assert torch.equal(first[2][k], second[2][k])


def test_device_resident_images_are_read_in_place_with_their_stride():
    c = C.case("noise_24x16")
    want = expected("noise_24x16", "fixed5", "rgb")["raw"]
    # a padded buffer: rows of 53 pixels inside rows of 57 (171 bytes, odd), offset by one pixel (3 bytes: unaligned base)
    wide = [torch.zeros((37, 57, 3), dtype=torch.uint8, device=DEV) for _ in range(2)]
    views = []
    for buf, img in zip(wide, (c["left"][0], c["right"][0])):
        buf[:, 1:54] = torch.from_numpy(img).to(DEV)
        views.append(buf[:, 1:54])
    assert views[0].stride() == (171, 3, 1) and views[0].data_ptr() % 4 == 3
    crop = RoICropper(c["cfg"])
    for _ in range(2):                      # the second call reuses the images already on the device
        left, right, _ = crop.generate(c["samples"], views[0], views[1], c["P_left"][0], c["P_right"][0], DEV, raw=True)
        assert np.array_equal(left.cpu().numpy(), want[0]) and np.array_equal(right.cpu().numpy(), want[1])
    # device-resident samples and projections as well
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    left, right, _ = crop.generate(dev(c["samples"]), views[0], views[1], dev(c["P_left"][0]), dev(c["P_right"][0]), DEV, raw=True)
    assert np.array_equal(left.cpu().numpy(), want[0]) and np.array_equal(right.cpu().numpy(), want[1])


def test_no_samples_give_empty_tensors():
    c = C.case("noise_24x16")
    left, right, meta = RoICropper(c["cfg"]).generate(np.zeros((0, 7)), c["left"][0], c["right"][0], c["P_left"][0], c["P_right"][0], DEV)
    assert left.shape == right.shape == (0, 3, 16, 24) and left.dtype == torch.float32 and left.device.type == "cuda"
    assert meta["trans_l"].shape == (0, 2, 3) and meta["kpts_2d_r"].shape == (0, 9, 2) and meta["kpts_2d_l_local"].shape == (0, 9, 2)


def test_device_transforms_feed_the_grid_projector():
    c = C.case("two_frames")
    keep = [i for i in range(len(c["samples"])) if c["frame"][i] == 0]     # GridProjector takes one calibration per call
    samples = c["samples"][keep]
    _, _, meta = RoICropper(c["cfg"]).generate(samples, c["left"][0], c["right"][0], c["P_left"][0], c["P_right"][0], DEV)
    grid = GridProjector(type("Cfg", (), dict(x_range=(-0.9, 0.9), y_range=(-0.8, 0.8), z_range=(-2.0, 2.0), grid_resolution=(3, 5, 7))))
    assert meta["trans_l"].is_cuda and meta["trans_l"].dtype == torch.float64
    on_device = grid.generate(samples, c["P_left"][0], c["P_right"][0], meta["trans_l"], meta["trans_r"], DEV)
    from_host = grid.generate(samples, c["P_left"][0], c["P_right"][0], meta["trans_l"].cpu().numpy(), meta["trans_r"].cpu().numpy(), DEV)
    for a, b in zip(on_device, from_host):
        assert a.shape == (len(keep), 2, 105) and torch.equal(a, b)
    # the projected grid lands inside the crop it was made for: the chain is consistent
    assert float(on_device[0][:, 0].min()) > 0 and float(on_device[0][:, 0].max()) < c["cfg"].resolution[0]


def test_error_paths():
    c = C.case("two_frames")
    crop = RoICropper(c["cfg"])
    args = (c["samples"], c["left"], c["right"], c["P_left"], c["P_right"])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        crop.generate(*args, "cpu", frame=c["frame"])
    for bad in (2, -1):
        frame = c["frame"].copy()
        frame[3] = bad
        with pytest.raises(ValueError, match="frame must index the 2 frames"):
            crop.generate(*args, DEV, frame=frame)
    with pytest.raises(ValueError, match="several frames need frame"):
        crop.generate(*args, DEV)
    with pytest.raises(ValueError, match="interpolation"):
        crop.generate(*args, DEV, frame=c["frame"], interpolation="cubic")
    with pytest.raises(ValueError, match="uint8"):
        crop.generate(c["samples"][:1], c["left"][0].astype(np.float32), c["right"][0], c["P_left"][0], c["P_right"][0], DEV)
