"""Golden vectors of the DSGN image backbone by IMPORTING THE REFERENCE (needs the reference checkout; CPU only):
    python tests/golden/make_golden_dsgn.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Builds the reference's own snvc.models.submodule.feature_extraction for each configuration of tests/dsgn_cases.py, seeds
its weights with benchlib.common.seeded_state and its input from numpy.random.default_rng, and stores only what the tests
cannot regenerate (two files, each below 1 MiB: tests/golden/dsgn_ref.npz and dsgn_ref_gn.npz):

    keys/<backbone>, shapes/<backbone>      ordered state-dict keys of every backbone with the default switches; shapes
                                            padded with -1 to four dimensions (dsgn_ref.npz)
    keys/<name>, shapes/<name>              the same for each golden configuration
    out/<name>, rpn/<name>                  eval output_feature / rpn_feature of that configuration on its seeded input
                                            (output_feature: its first dsgn_cases.STORED_CHANNELS[name] channels, if listed)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for _m in ("cv2",):
    sys.modules.setdefault(_m, types.ModuleType(_m))
sys.path.insert(0, REF)

import snvc.models.submodule as ref_sub  # noqa: E402

from benchlib.common import seeded_state  # noqa: E402
import dsgn_cases as DC  # noqa: E402

torch.set_num_threads(8)


def layout(m):
    sd = m.state_dict()
    return np.array(list(sd)), np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], np.int32)


def solid(name, t):
    a = t.detach().numpy()
    assert np.isfinite(a).all() and np.abs(a).max() > 0, name
    print(f"{name:24s} {tuple(a.shape)}  max |v| {np.abs(a).max():.4g}")
    return a


files = {f: {} for f in DC.FILES}
with torch.no_grad():
    for bb in DC.BACKBONES:
        files["dsgn_ref.npz"][f"keys/{bb}"], files["dsgn_ref.npz"][f"shapes/{bb}"] = layout(ref_sub.feature_extraction(DC.cfg(backbone=bb)))
    for fname, names in DC.FILES.items():
        out = files[fname]
        for nm in names:
            fields, shape, wseed, xseed = DC.GOLDEN[nm]
            m = ref_sub.feature_extraction(DC.cfg(**fields))
            out[f"keys/{nm}"], out[f"shapes/{nm}"] = layout(m)
            m.load_state_dict(seeded_state(m, wseed), strict=True)
            feat, rpn = m.eval()(DC.image(shape, xseed))
            if feat is not None:
                out[f"out/{nm}"] = solid(f"out/{nm}", feat[:, :DC.STORED_CHANNELS.get(nm, feat.size(1))])
            if rpn is not None:
                out[f"rpn/{nm}"] = solid(f"rpn/{nm}", rpn)
for fname, out in files.items():
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
