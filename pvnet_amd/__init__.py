"""PVNet's inference side on AMD Instinct: see README.md for the modules.

The ground-truth side (pvnet_amd/render.py), model preparation (pvnet_amd/models.py), the training
loss (pvnet_amd/net_utils.py) and the training augmentation (pvnet_amd/augment.py) are exported here, resolved on first use so that importing the package
stays as cheap as it was.  The augmentation's hot-path entry point keeps its module's name in
front of it, ``pvnet_amd.augment.apply``: a bare ``apply`` at package level would say nothing.  So do
the frame composition's two (pvnet_amd/compose.py): ``pvnet_amd.compose.compose`` and
``pvnet_amd.compose.finish``; the rest of that module is exported here.  The optimiser step
(pvnet_amd/optim.py) exports its one class, ``Optimizer``.  Scoring in the BOP Challenge's terms
(pvnet_amd/bop.py) exports its table, its two error entries and the average recall.  ``vsd`` and
``sym_errors`` are functions, so ``pvnet_amd.bop`` the module stays reachable under its own name.  Depth
pose refinement (pvnet_amd/icp.py) exports ``refine_depth``; ``pvnet_amd.icp.iterate`` and
``pvnet_amd.icp.linearise`` keep the module's name in front of them."""

_RENDER = ("MeshTable", "render_labels", "vertex_field", "render_ground_truth", "mask_iou")
_MODELS = ("extent", "farthest_points", "diameter", "corners_3d", "keypoints_3d")
_LOSS = ("pvnet_loss",)
_AUGMENT = ("AugmentParams", "label_stats", "random_params", "transform_keypoints", "augment_ground_truth")
_COMPOSE = ("Placement", "make_picks", "random_placement", "shift_keypoints", "shift_camera", "visible_fraction",
            "compose_ground_truth")
_OPTIM = ("Optimizer",)
_BOP = ("SymmetryTable", "sym_errors", "vsd", "average_recall")
_ICP = ("refine_depth",)
__all__ = [*_RENDER, *_MODELS, *_LOSS, *_AUGMENT, *_COMPOSE, *_OPTIM, *_BOP, *_ICP]


def __getattr__(name):
    if name in _RENDER:
        from . import render
        return getattr(render, name)
    if name in _MODELS:
        from . import models
        return getattr(models, name)
    if name in _LOSS:
        from . import net_utils
        return getattr(net_utils, name)
    if name in _AUGMENT:
        from . import augment
        return getattr(augment, name)
    if name in _COMPOSE:
        from . import compose
        return getattr(compose, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _BOP:
        from . import bop
        return getattr(bop, name)
    if name in _ICP:
        from . import icp
        return getattr(icp, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
