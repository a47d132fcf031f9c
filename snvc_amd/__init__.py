"""snvc_amd -- MI355X (gfx950) implementation of SNVC's cost-volume / voxel-resampling /
3D-CNN hot path behind the reference's own operator API.

    snvc_amd.extension.build_cost_volume   <->  snvc.extension.build_cost_volume
    snvc_amd.extension.roiaware_pool3d     <->  snvc.extension.roiaware_pool3d
    snvc_amd.extension.iou3d_nms           <->  snvc.extension.iou3d_nms
    snvc_amd.models.submodule              <->  snvc.models.submodule (3D blocks)
    snvc_amd.models.vernier                <->  snvc.models.vernier   (VernierScale 3D trunk)
    snvc_amd.models.hrnet                  <->  snvc.models.hrnet     (HRNet backbone; install_as_snvc(backbone="hip"))
    snvc_amd.models.loss3d                 <->  snvc.models.loss3d    (training losses)
    snvc_amd.models.FCmodel                <->  snvc.models.FCmodel   (the FC box head of use_bbox_head)
    snvc_amd.thirdparty.oriented_iou_loss  <->  snvc.thirdparty.oriented_iou_loss (the IoU losses' geometry; upstream never shipped it)

Everything executes in hand-written HIP kernels from ``libsnvc_hip.so`` (C ABI:
``include/snvc_hip.h``, ``include/snvc_iou3d.h``, ``include/snvc_hrnet.h``).  There is no CPU path: CPU tensors raise, and a missing shared
library raises at first use.  The exceptions are the losses (``models.loss3d``, ``models.iou_loss``,
``thirdparty.oriented_iou_loss``), whose CPU and float64 inputs take a torch route written from the same definitions.
"""
__version__ = "0.1.0"

# reference module name -> the module of this package that stands in for it
_ALIASES = {
    "snvc.extension.build_cost_volume": "snvc_amd.extension.build_cost_volume",
    "snvc.extension.roiaware_pool3d.roiaware_pool3d_utils": "snvc_amd.extension.roiaware_pool3d.roiaware_pool3d_utils",
    "snvc.extension.iou3d_nms.iou3d_nms_utils": "snvc_amd.extension.iou3d_nms.iou3d_nms_utils",
    "snvc.models.submodule": "snvc_amd.models.submodule",
    "snvc.models.vernier": "snvc_amd.models.vernier",
    "snvc.models.loss3d": "snvc_amd.models.loss3d",
    "snvc.models.FCmodel": "snvc_amd.models.FCmodel",
    "snvc.thirdparty.oriented_iou_loss": "snvc_amd.thirdparty.oriented_iou_loss",
}


def install_as_snvc(backbone=True):
    """Make the reference's own import lines resolve to this package: after ``snvc_amd.install_as_snvc()`` (once, before
    the reference's modules are imported) ``from snvc.models.vernier import get_model``,
    ``from snvc.extension.build_cost_volume import build_cost_volume`` ... give the MI355X implementations, while every
    other ``snvc.*`` module (dataset, utils; HRNet unless ``backbone="hip"``) still comes from the reference checkout on
    ``sys.path``.  ``backbone=True`` also wires ``snvc.models.hrnet.get_model`` into ``VernierScale`` as its feature
    extractor factory when the reference package is importable (vernier.py:57-66), so that
    ``tools/inference_agnostic.py`` runs with no edit but its DataParallel line.
    ``backbone="hip"`` aliases ``snvc.models.hrnet`` to ``snvc_amd.models.hrnet`` as well, so that the backbone runs on
    the HIP kernels too and no reference module is needed for the model."""
    import importlib
    import sys
    for ref_name, ours in _ALIASES.items():
        mod = importlib.import_module(ours)
        sys.modules[ref_name] = mod
        parent, _, leaf = ref_name.rpartition(".")
        if parent in sys.modules:                       # `import snvc.models.vernier as v` reads the attribute chain
            setattr(sys.modules[parent], leaf, mod)
    if backbone == "hip":
        mod = importlib.import_module("snvc_amd.models.hrnet")
        sys.modules["snvc.models.hrnet"] = mod
        try:                                            # `import snvc.models.hrnet as h` reads the attribute chain
            setattr(importlib.import_module("snvc.models"), "hrnet", mod)
        except ImportError:                             # no reference checkout: `from snvc.models.hrnet import ...` still works
            pass
    if backbone:
        try:
            hrnet = importlib.import_module("snvc.models.hrnet")
        except Exception:
            return
        vernier = sys.modules["snvc.models.vernier"]
        vernier.get_feat_extraction = lambda cfg, is_train=False, **kw: hrnet.get_model(cfg, is_train, **kw)
