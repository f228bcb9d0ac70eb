"""PVNet's inference side on AMD Instinct: see README.md for the modules.

The ground-truth side (pvnet_amd/render.py), model preparation (pvnet_amd/models.py) and the training
loss (pvnet_amd/net_utils.py) are exported here, resolved on first use so that importing the package
stays as cheap as it was."""

_RENDER = ("MeshTable", "render_labels", "vertex_field", "render_ground_truth", "mask_iou")
_MODELS = ("extent", "farthest_points", "diameter", "corners_3d", "keypoints_3d")
_LOSS = ("pvnet_loss",)
__all__ = [*_RENDER, *_MODELS, *_LOSS]


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
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
