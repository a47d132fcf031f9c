"""The descriptors and launch cells behind tests/golden/f16_plan_table.json and tests/golden/f16_plan_gpu.json: what the host side
of snvc_amd/csrc/conv3d_f16.hip decides for a layer (packed bytes, statistics workspace, accepted or rejected and with which words)
and what its launches compute, recorded from the library of the commit before that file's kernel forms became records
(tests/golden/make_golden_f16_plan.py) and held to that record by tests/test_f16_plan_host.py and tests/test_gpu_f16_plan.py."""
import ctypes
import hashlib

import numpy as np

from snvc_amd import _lib
from split_format import split_pair

SERIAL, NARROW, SMALL, Q16 = _lib.ALGO_X3_SERIAL, _lib.ALGO_X3_NARROW, _lib.ALGO_X3_SMALL, _lib.ALGO_X3_Q16
ALGOS = [0, SERIAL, NARROW, SMALL, Q16]
T = (3, 2, 1, 1)      # the transposed layer: (ksize, stride, dilation, transposed)
KEYS = [(1, 1, 1), (3, 1, 1), (3, 2, 1), (5, 1, 1), (5, 1, 2), (7, 1, 1), T]
CINS = [8, 16, 24, 64, 12]
COUTS = [1, 32, 64, 96, 33]
FIELDS = ["N", "Cin", "Din", "Hin", "Win", "Cout", "Dout", "Hout", "Wout", "ksize", "stride", "dilation", "pad", "transposed", "algo"]
PROBES = ["snvc_f16_conv3d_packed_weight_bytes", "snvc_f16x3_conv3d_packed_weight_bytes", "snvc_f16x3_conv3d_stats_workspace_bytes"]

# Every form record of conv3d_f16.hip (FORM_<name>): split mode or fp16 storage, the layer key, and a (Cout, algo) that selects it.
FORMS = {
    "K7QN": (False, (7, 1, 1), 32, Q16), "K5QN": (False, (5, 1, 1), 32, Q16), "K5D2QN": (False, (5, 1, 2), 32, Q16),
    "K7Q": (False, (7, 1, 1), 64, Q16), "K5Q": (False, (5, 1, 1), 64, Q16), "K5D2Q": (False, (5, 1, 2), 64, Q16),
    "K1": (False, (1, 1, 1), 64, 0), "K3": (False, (3, 1, 1), 64, 0), "K3H": (False, (3, 1, 1), 1, 0), "K3S2": (False, (3, 2, 1), 64, 0),
    "K5": (False, (5, 1, 1), 64, 0), "K5D2": (False, (5, 1, 2), 64, 0), "K7": (False, (7, 1, 1), 64, 0), "DC": (False, T, 64, 0),
    "K1N": (False, (1, 1, 1), 32, 0), "K3N": (False, (3, 1, 1), 32, 0), "K3S2N": (False, (3, 2, 1), 32, 0), "K5N": (False, (5, 1, 1), 32, 0),
    "K5D2N": (False, (5, 1, 2), 32, 0), "K7N": (False, (7, 1, 1), 32, 0), "DCN": (False, T, 32, 0),
    "K3X": (True, (3, 1, 1), 32, 0), "K3X2": (True, (3, 1, 1), 64, 0), "K3XS": (True, (3, 1, 1), 32, SERIAL), "K3X2S": (True, (3, 1, 1), 64, SERIAL),
    "K3XT": (True, (3, 1, 1), 32, SMALL), "K3S2X": (True, (3, 2, 1), 64, 0), "K3S2XT": (True, (3, 2, 1), 64, SMALL), "DCX": (True, T, 64, 0),
    "DCXT": (True, T, 64, SMALL), "DCXN": (True, T, 32, 0), "K1X": (True, (1, 1, 1), 32, 0), "K5X": (True, (5, 1, 1), 32, 0),
    "K5D2X": (True, (5, 1, 2), 32, 0), "K7X": (True, (7, 1, 1), 32, 0), "K3XH": (True, (3, 1, 1), 1, 0), "K5XQ": (True, (5, 1, 1), 32, Q16),
    "K5D2XQ": (True, (5, 1, 2), 32, Q16), "K7XQ": (True, (7, 1, 1), 32, Q16), "K3S2XQ": (True, (3, 2, 1), 64, Q16), "K3XQ": (True, (3, 1, 1), 32, Q16),
}


def desc(key, cin, cout, algo=0, ext=(9, 10, 33), n=1, **over):
    """The descriptor fields of a layer of ``key`` on an input of extents ``ext``."""
    k, s, dil = key[:3]
    if len(key) == 4:
        pad, out = 1, [2 * e for e in ext]
    else:
        pad = dil * (k - 1) // 2
        out = [(e + 2 * pad - dil * (k - 1) - 1) // s + 1 for e in ext]
    d = dict(N=n, Cin=cin, Din=ext[0], Hin=ext[1], Win=ext[2], Cout=cout, Dout=out[0], Hout=out[1], Wout=out[2], ksize=k, stride=s,
             dilation=dil, pad=pad, transposed=int(len(key) == 4), algo=algo)
    d.update(over)
    return d


def plan_cases():
    """(tag, fields): every key x Cin x Cout x algo; other extents and batch sizes at Cin 16; the rejected descriptors."""
    for key in KEYS:
        for cout in COUTS:
            for algo in ALGOS:
                for cin in CINS:
                    yield "grid", desc(key, cin, cout, algo)
                yield "grid", desc(key, 16, cout, algo, ext=(1, 1, 1))
                for n in (0, 2):
                    yield "grid", desc(key, 16, cout, algo, n=n)
    for split_cout in (32, 64):
        yield "rejected", desc((3, 1, 1), 16, split_cout, pad=0)                      # wrong pad
        yield "rejected", desc((3, 1, 1), 16, split_cout, Wout=32)                    # wrong output size
        yield "rejected", desc((3, 2, 1), 16, split_cout, Dout=9)
        yield "rejected", desc(T, 16, split_cout, Hout=19)
        yield "rejected", desc(T, 16, split_cout, pad=0)
        yield "rejected", desc((3, 1, 1), 16, split_cout, n=65536)                    # N > 65535
        yield "rejected", desc((3, 1, 1), 16, split_cout, n=-1)
        yield "rejected", desc((3, 1, 1), 16, split_cout, Win=0)
        yield "rejected", desc((3, 1, 2), 16, split_cout)                             # no such key
        yield "rejected", desc((5, 2, 1), 16, split_cout)
    yield "half rejected", desc((3, 2, 1), 16, 32)                                    # stride 2 with Cout 32: fp16 storage only
    yield "rejected", desc(T, 16, 48)                                                 # transposed with Cout 48
    yield "rejected", desc(T, 16, 1)
    yield "rejected", desc((3, 1, 1), 0, 32)


def probe(L, fields):
    """[value, error text or ""] of each of PROBES on one descriptor."""
    d = _lib.Conv3dDesc(**fields)
    row = []
    for name in PROBES:
        v = int(getattr(L, name)(ctypes.byref(d)))
        row += [v, L.snvc_last_error_string().decode() if v < 0 else ""]
    return row


def null_calls(L, F):
    """[entry point, case, status, error text]: a null descriptor, a descriptor with null pointers and an empty batch on each of the
    five split entry points and on snvc_f16_conv3d_forward.  Nothing is launched."""
    n = None
    out = []
    for case, d in (("null desc", None), ("null pointers", _lib.Conv3dDesc(**desc((3, 1, 1), 16, 32, Q16))),
                    ("null pointers, transposed", _lib.Conv3dDesc(**desc(T, 16, 32))), ("empty batch", _lib.Conv3dDesc(**desc((3, 1, 1), 16, 32, n=0)))):
        p = ctypes.byref(d) if d is not None else None
        calls = {
            "snvc_f16_conv3d_forward": lambda: L.snvc_f16_conv3d_forward(p, n, n, n, n, n, n, n, n),
            "snvc_f16x3_conv3d_forward": lambda: L.snvc_f16x3_conv3d_forward(p, n, n, n, n, n, n, n, n, n, n, n, n, 1.0, 1.0, n, n),
            "snvc_f16x3_conv3d_forward_f32": lambda: L.snvc_f16x3_conv3d_forward_f32(p, n, n, n, n, n, n, n, n, 1.0, n),
            "snvc_f16x3_conv3d_forward_stats": lambda: L.snvc_f16x3_conv3d_forward_stats(p, n, n, n, n, n, n, n, 1.0, n, n, n, n, n, n, n, 1e-5, n),
            "snvc_f16x3_deconv3d_tail_forward": lambda: L.snvc_f16x3_deconv3d_tail_forward(p, n, n, n, n, n, n, n, 1.0, n, n, 1.0, n, n),
            "snvc_fused_first_conv3d_forward": lambda: F.snvc_fused_first_conv3d_forward(p, n, n, n, n, n, n, n, 1.0, n, n, 0, 0, n, n, n, 1, 0, 0, 0, 0, n),
        }
        for name, call in calls.items():
            rc = int(call())
            out.append([name, case, rc, L.snvc_last_error_string().decode() if rc else ""])
    return out


# ---------------------------------------------------------------------------------------------- launches (GPU)
KINDS = ["split", "f32", "f32+res_f32", "res pre", "res post", "head", "stats", "tail"]      # of a split form
PLAIN_KINDS = ["c8", "c8 res post"]                                                           # of an fp16-storage form
RELU, ADD_PRE, ADD_POST = _lib.EPI_RELU, _lib.EPI_ADD_PRE, _lib.EPI_ADD_POST


def gpu_extents(key):
    """The smallest input extents with more than one tile and a ragged edge; dilated 5^3: four parity classes of four sizes."""
    if len(key) == 4:
        return (3, 4, 17)
    return (6, 8, 34) if key[1] == 2 else (6, 6, 33) if key[2] == 2 else (5, 6, 33)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_form(name, torch, dev, x_pad=0):
    """{kind: [status, text, {buffer: sha256}]} of every call kind on form ``name``, plus "packed": the sha256 of its packed weights.
    Inputs from a numpy seed fixed per form; N = 2; ``x_pad``: extra elements between the samples of x (a non-default batch stride)."""
    from snvc_amd import _fused
    L, F = _lib.lib(), _fused.lib()
    split, key, cout, algo = FORMS[name]
    cin, n, ext = 16, 2, gpu_extents(key)
    base = desc(key, cin, cout, algo, ext=ext, n=n)
    in_sp = int(np.prod(ext))
    out_ext = (base["Dout"], base["Hout"], base["Wout"])
    out_sp = int(np.prod(out_ext))
    r = np.random.default_rng(1000 + sorted(FORMS).index(name))
    k3 = 27 if base["transposed"] else key[0] ** 3
    w = (r.standard_normal((cout * cin * k3,)) / np.sqrt(cin * k3)).astype(np.float32)

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    def pair(shape_c, sp, pad=0):          # [N][2][C/8][sp][8] halves (+ pad per sample), value = hi + lo
        v = r.standard_normal((n, shape_c // 8, sp, 8)).astype(np.float32)
        hi, lo = split_pair(v, 1.0)
        buf = np.zeros((n, 2 * shape_c * sp + pad), np.float16)
        buf[:, :shape_c * sp] = hi.reshape(n, -1)
        buf[:, shape_c * sp:2 * shape_c * sp] = lo.reshape(n, -1)
        return torch.from_numpy(buf).to(dev)

    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    lo_ptr = lambda t, c, sp: ctypes.c_void_p(t.data_ptr() + 2 * c * sp) if t is not None else None      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    err = lambda rc: L.snvc_last_error_string().decode() if rc else ""      # noqa: E731
    wt = dev_f32(w)
    d0 = _lib.Conv3dDesc(**base)
    nbytes = int((L.snvc_f16x3_conv3d_packed_weight_bytes if split else L.snvc_f16_conv3d_packed_weight_bytes)(ctypes.byref(d0)))
    assert nbytes > 0, (name, L.snvc_last_error_string().decode())
    packed = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    rc = (L.snvc_f16x3_conv3d_pack_weights(ctypes.byref(d0), ptr(wt), ptr(packed), 4.0, stream) if split
          else L.snvc_f16_conv3d_pack_weights(ctypes.byref(d0), ptr(wt), ptr(packed), stream))
    assert rc == 0, (name, err(rc))
    got = {"packed": _sha(packed)}
    scale, bias = dev_f32(r.uniform(0.5, 1.5, max(cout, 8))), dev_f32(r.standard_normal(max(cout, 8)))
    ccout = max(cout, 8)     # buffers of a one-channel layer that is asked for a C8 result: one channel group, never written

    if not split:
        x = torch.from_numpy(r.standard_normal((n, cin * in_sp)).astype(np.float16)).to(dev)
        res = torch.from_numpy(r.standard_normal((n, ccout * out_sp)).astype(np.float16)).to(dev)
        for kind in PLAIN_KINDS:
            flags = RELU | (ADD_POST if kind == "c8 res post" else 0)
            d = _lib.Conv3dDesc(**dict(base, flags=flags))
            y = torch.zeros((n, ccout * out_sp), dtype=torch.float16, device=dev)
            y32 = torch.zeros((n, out_sp), dtype=torch.float32, device=dev)
            rc = int(L.snvc_f16_conv3d_forward(ctypes.byref(d), ptr(x), ptr(packed), ptr(scale), ptr(bias), ptr(res) if flags & ADD_POST else None,
                                               ptr(y), ptr(y32) if cout == 1 else None, stream))
            got[kind] = [rc, err(rc), {} if rc else {"y": _sha(y), "y_f32": _sha(y32)}]
        return got

    x = pair(cin, in_sp, x_pad)
    res = pair(ccout, out_sp)
    res32 = dev_f32(r.standard_normal((n, ccout * out_sp)))
    head = dev_f32(r.standard_normal(32))
    x_mul = dev_f32([2.0])
    gamma, beta = dev_f32(r.uniform(0.5, 1.5, ccout)), dev_f32(r.standard_normal(ccout))
    tail_packed = None
    if cout % 32 == 0:
        tail_packed = torch.zeros(int(L.snvc_f16x3_tail_packed_weight_bytes(cout)), dtype=torch.uint8, device=dev)
        tw = dev_f32(r.standard_normal(cout * 27) / 8)
        rc = L.snvc_f16x3_tail_pack_weights(ptr(tw), cout, ptr(tail_packed), 2.0, stream)
        assert rc == 0, (name, err(rc))
    xbs = 2 * cin * in_sp + x_pad if x_pad else 0
    for kind in KINDS:
        flags = {"res pre": RELU | ADD_PRE, "res post": RELU | ADD_POST, "tail": RELU | ADD_POST, "stats": 0}.get(kind, RELU)
        d = _lib.Conv3dDesc(**dict(base, flags=flags, x_batch_stride=xbs))
        y = torch.zeros((n, 2 * ccout * out_sp), dtype=torch.float16, device=dev)
        y32 = torch.zeros((n, ccout * out_sp), dtype=torch.float32, device=dev)
        y_head = torch.zeros((n, out_sp), dtype=torch.float32, device=dev)
        t_out = torch.zeros((n, 27 * 8 * in_sp), dtype=torch.float32, device=dev)
        rows = torch.zeros((4, ccout), dtype=torch.float32, device=dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        xa = (ptr(x), lo_ptr(x, cin, in_sp), ptr(packed), ptr(scale), ptr(bias))
        plane = cout == 1
        if kind in ("split", "res pre", "res post", "head"):
            withres, withhead = kind.startswith("res"), kind == "head"
            # a one-channel layer writes the fp32 plane: "split" is then its plane call, the other kinds stay as they are (and are rejected)
            to_plane = plane and kind == "split"
            rc = L.snvc_f16x3_conv3d_forward(ctypes.byref(d), *xa, ptr(res) if withres else None, lo_ptr(res, ccout, out_sp) if withres else None,
                                             None if to_plane else ptr(y), None if to_plane else lo_ptr(y, ccout, out_sp), ptr(y32) if to_plane else None,
                                             ptr(head) if withhead else None, ptr(y_head) if withhead else None, 0.5, 2.0, ptr(overflow), stream)
        elif kind == "f32":
            rc = L.snvc_f16x3_conv3d_forward(ctypes.byref(d), *xa, None, None, None, None, ptr(y32), None, None, 0.5, 1.0, ptr(overflow), stream)
        elif kind == "f32+res_f32":
            rc = L.snvc_f16x3_conv3d_forward_f32(ctypes.byref(d), *xa, ptr(x_mul), ptr(res32), ptr(y32), 0.5, stream)
        elif kind == "stats":
            ws_bytes = int(L.snvc_f16x3_conv3d_stats_workspace_bytes(ctypes.byref(d)))
            ws = torch.zeros(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
            rc = L.snvc_f16x3_conv3d_forward_stats(ctypes.byref(d), *xa, ptr(x_mul), ptr(y32), 0.5, ptr(gamma), ptr(beta), ptr(rows[0]), ptr(rows[1]),
                                                   ptr(rows[2]), ptr(rows[3]), ptr(ws), 1e-5, stream)
        else:
            rc = L.snvc_f16x3_deconv3d_tail_forward(ctypes.byref(d), *xa, ptr(res), lo_ptr(res, ccout, out_sp), 2.0, ptr(tail_packed), ptr(t_out), 0.25,
                                                    ptr(overflow), stream)
        rc = int(rc)
        torch.cuda.synchronize(dev)
        got[kind] = [rc, err(rc), {} if rc else {"y": _sha(y), "y_f32": _sha(y32), "y_head": _sha(y_head), "t_out": _sha(t_out), "stats": _sha(rows),
                                                 "overflow": _sha(overflow)}]
    return got
