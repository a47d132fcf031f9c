"""Writes tests/golden/packed_count_table.json: what ``snvc_conv3d_packed_weight_count`` returns over a grid of layer descriptors.

    SNVC_HIP_LIB=<libsnvc_hip.so of the recording commit> python tests/golden/make_golden_packed_count.py

Run it ONLY against a library built from the parent of the commit that gave conv3d.hip its ``PackedLayout`` (the commit that
added this file), or at that parent: the table is a record of what the hand-written count returned there, which
tests/test_packed_count_host.py holds the function to.  The call takes a descriptor and nothing else: no device is needed.

The grid: every (ksize, stride, dilation) key of ``make_plan`` -- cubic, transposed, depth-1 (3 x 7 and dilation 2 among them)
and depth-1 transposed -- with Cout and Cin each in {1, 2, 3, 31, 32, 33, 64, 96}, and descriptors the function rejects (-1;
the error text is recorded with them).  The file holds the descriptor fields' names and one row per descriptor: the fields, the
count, and for a rejected one the error text.  The script asserts that each of the three raw-tail cases and each of the five
Winograd packings occurs among the accepted rows (the raw tails by what they add to the count, the packings by the descriptor
fields that select them).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from snvc_amd import _lib  # noqa: E402

FIELDS = ["N", "Cin", "Din", "Hin", "Win", "Cout", "Dout", "Hout", "Wout", "ksize", "stride", "dilation", "pad", "transposed",
          "ksize_d", "ksize_h"]
CHANNELS = [1, 2, 3, 31, 32, 33, 64, 96]
CUBIC_KEYS = [(1, 1, 1), (3, 1, 1), (3, 2, 1), (5, 1, 1), (5, 1, 2), (7, 1, 1)]
# depth-1 layers: (ksize, stride, dilation, ksize_h); ksize_h = 0 means ksize
PLANAR_KEYS = [(1, 1, 1, 0), (1, 2, 1, 0), (3, 1, 1, 0), (3, 1, 1, 3), (3, 2, 1, 0), (7, 1, 1, 3), (3, 1, 2, 0)]


def cubic(cout, cin, k, s, dil, din=9, hin=10, win=20, n=1, **over):
    pad = dil * (k - 1) // 2
    eff = dil * (k - 1) + 1
    o = [(e + 2 * pad - eff) // s + 1 for e in (din, hin, win)]
    d = dict(N=n, Cin=cin, Din=din, Hin=hin, Win=win, Cout=cout, Dout=o[0], Hout=o[1], Wout=o[2], ksize=k, stride=s, dilation=dil,
             pad=pad, transposed=0, ksize_d=0, ksize_h=0)
    d.update(over)
    return d


def transposed(cout, cin, din=5, hin=6, win=8, **over):
    d = dict(N=1, Cin=cin, Din=din, Hin=hin, Win=win, Cout=cout, Dout=2 * din, Hout=2 * hin, Wout=2 * win, ksize=3, stride=2,
             dilation=1, pad=1, transposed=1, ksize_d=0, ksize_h=0)
    d.update(over)
    return d


def planar(cout, cin, k, s, dil, kh, hin=36, win=40, **over):
    khe = kh or k
    if dil == 2:
        pad, ho, wo = 2, hin, win
    else:
        pad = (k - 1) // 2
        ho, wo = (hin + 2 * ((khe - 1) // 2) - khe) // s + 1, (win + 2 * pad - k) // s + 1
    d = dict(N=2, Cin=cin, Din=1, Hin=hin, Win=win, Cout=cout, Dout=1, Hout=ho, Wout=wo, ksize=k, stride=s, dilation=dil, pad=pad,
             transposed=0, ksize_d=1, ksize_h=kh)
    d.update(over)
    return d


def cases():
    """(tag, descriptor) pairs; the tag names the family a row was built for."""
    for cout in CHANNELS:
        for cin in CHANNELS:
            for k, s, dil in CUBIC_KEYS:
                yield f"cubic k{k} s{s} d{dil}", cubic(cout, cin, k, s, dil)
            yield "transposed", transposed(cout, cin)
            yield "transposed depth-1", transposed(cout, cin, din=1, Dout=1, ksize_d=1)
            for k, s, dil, kh in PLANAR_KEYS:
                yield f"depth-1 k{k} s{s} d{dil} kh{kh}", planar(cout, cin, k, s, dil, kh)
    # the count does not depend on the extents or the batch: odd extents, an empty batch, a small depth-1 image
    yield "cubic k3 s1 d1", cubic(32, 32, 3, 1, 1, din=1, hin=1, win=1)
    yield "cubic k3 s1 d1", cubic(33, 3, 3, 1, 1, din=7, hin=5, win=3, n=0)
    yield "cubic k3 s2 d1", cubic(64, 31, 3, 2, 1, din=7, hin=5, win=3)
    yield "depth-1 k3 s1 d1 kh0", planar(64, 64, 3, 1, 1, 0, hin=8, win=12)
    yield "transposed depth-1", transposed(32, 64, din=1, Dout=1, ksize_d=1, ksize_h=3)
    # rejected descriptors
    yield "rejected", cubic(32, 32, 3, 1, 1, N=-1)
    yield "rejected", cubic(32, 0, 3, 1, 1)
    yield "rejected", cubic(0, 32, 3, 1, 1)
    yield "rejected", cubic(32, 32, 3, 1, 1, Win=0)
    yield "rejected", cubic(32, 32, 3, 1, 2)                       # (3,1,2) is no cubic key
    yield "rejected", cubic(32, 32, 5, 2, 1)
    yield "rejected", cubic(32, 32, 7, 1, 2)
    yield "rejected", cubic(32, 32, 2, 1, 1)
    yield "rejected", cubic(32, 32, 3, 1, 1, pad=0)
    yield "rejected", cubic(32, 32, 3, 1, 1, Wout=19)
    yield "rejected", cubic(32, 32, 3, 2, 1, Dout=9)
    yield "rejected", cubic(32, 32, 3, 1, 1, ksize_d=2)
    yield "rejected", cubic(32, 32, 3, 1, 1, ksize_h=1)
    yield "rejected", cubic(64 * 65535 + 1, 1, 1, 1, 1, din=1, hin=1, win=1)     # more than 65535 channel groups
    yield "rejected", cubic(32, 32, 3, 1, 1, N=65536)
    yield "rejected", transposed(32, 32, ksize=5, pad=2)
    yield "rejected", transposed(32, 32, stride=1)
    yield "rejected", transposed(32, 32, dilation=2)
    yield "rejected", transposed(32, 32, Dout=9)
    yield "rejected", transposed(32, 32, din=1, Dout=2, ksize_d=1)
    yield "rejected", transposed(32, 32, din=1, Dout=1, ksize_d=1, ksize_h=7)
    yield "rejected", planar(32, 32, 3, 1, 1, 0, Din=2, Dout=2)
    yield "rejected", planar(32, 32, 3, 1, 1, 0, pad=0)
    yield "rejected", planar(32, 32, 3, 2, 2, 0)                   # dilation 2 is built for stride 1 only
    yield "rejected", planar(32, 32, 3, 1, 2, 3)                   # ... and for ksize_h = 0
    yield "rejected", planar(32, 32, 3, 1, 1, 1)
    yield "rejected", planar(32, 32, 7, 1, 1, 0)                   # depth-1 ksize 7 is the 3 x 7 layer only
    yield "rejected", planar(32, 32, 7, 2, 1, 3)
    yield "rejected", planar(32, 32, 5, 1, 1, 0)
    yield "rejected", planar(32, 32, 3, 1, 1, 0, Hout=35)


def main():
    L = _lib.lib()
    rows, tags = [], {}
    for tag, fields in cases():
        d = _lib.Conv3dDesc(**fields)
        count = int(L.snvc_conv3d_packed_weight_count(ctypes.byref(d)))
        row = [fields[k] for k in FIELDS] + [count]
        if count < 0:
            assert count == -1 and tag == "rejected", (tag, fields, count)
            row.append(L.snvc_last_error_string().decode())
        else:
            assert tag != "rejected", fields
        tags.setdefault(tag, []).append((fields, count))
        rows.append(row)
    assert int(L.snvc_conv3d_packed_weight_count(None)) == -1        # a null descriptor: -1, no message of its own

    def count_of(tag, cout, cin):
        return next(c for f, c in tags[tag] if (f["Cout"], f["Cin"]) == (cout, cin) and f["Din"] in (9, 5, 1) and f["N"] in (1, 2))

    # the three raw-tail cases: the tail is what a one- (two-) channel layer holds beyond the MFMA and Winograd packings, which
    # are the same for every Cout <= 32 (one group) and every Cin in a chunk
    assert count_of("cubic k1 s1 d1", 2, 32) - count_of("cubic k1 s1 d1", 3, 32) == 2 * 32       # to <= 2 channels: [Cout][Cin]
    assert count_of("cubic k1 s1 d1", 31, 2) - count_of("cubic k1 s1 d1", 31, 3) == 31 * 2       # from <= 2 channels
    assert count_of("cubic k3 s1 d1", 1, 32) - count_of("cubic k3 s1 d1", 2, 32) == 32 * 27      # k3 to one channel: [Cin][27]
    assert count_of("transposed", 1, 32) - count_of("transposed", 2, 32) == 32 * 27              # transposed to one channel
    assert count_of("depth-1 k1 s1 d1 kh0", 1, 32) == count_of("depth-1 k1 s1 d1 kh0", 3, 32)    # depth-1 layers: never a tail
    assert count_of("transposed depth-1", 1, 32) == count_of("transposed depth-1", 2, 32)
    # the five Winograd packings (depth-1 k3 / stride 1, k3 / stride 2, k3, k5 -- dilation 2 too --, k7), known by the descriptor
    # fields that select them, and the layers that carry none
    def packing(f):
        if f["ksize_d"] == 1:
            return "depth-1" if (f["ksize"], f["stride"], f["dilation"], f["transposed"]) == (3, 1, 1, 0) else None
        if f["transposed"] or f["ksize"] == 1:
            return None
        return "k3s2" if f["stride"] == 2 else f"k{f['ksize']}"
    seen = {}
    for tag, got in tags.items():
        for f, c in got:
            if c >= 0:
                seen.setdefault(packing(f), set()).add(tag)
    assert set(seen) == {"depth-1", "k3s2", "k3", "k5", "k7", None}, seen
    assert {"cubic k5 s1 d1", "cubic k5 s1 d2"} <= seen["k5"] and {"depth-1 k3 s1 d1 kh0", "depth-1 k3 s1 d1 kh3"} <= seen["depth-1"]
    # a depth-1 k3 layer at dilation 2 has the direct section of the dilation-1 layer and no Winograd packing behind it
    assert count_of("depth-1 k3 s1 d1 kh0", 32, 32) > count_of("depth-1 k3 s1 d2 kh0", 32, 32)
    # the cubic k3 / stride 1 form takes four input channels per chunk, its Winograd packing two: a third channel grows only the latter
    assert count_of("cubic k3 s1 d1", 32, 3) > count_of("cubic k3 s1 d1", 32, 2) == count_of("cubic k3 s1 d1", 31, 1)
    assert len(tags["rejected"]) >= 25 and len({r[-1] for r in rows if r[len(FIELDS)] < 0}) >= 12   # many different messages

    out = os.path.join(HERE, "packed_count_table.json")
    with open(out, "w") as f:
        json.dump({"fields": FIELDS, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rows)} rows ({len(tags['rejected'])} rejected), {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
