"""PVNet's inference side on AMD Instinct: see README.md for the modules.

The ground-truth side (pvnet_amd/render.py) and model preparation (pvnet_amd/models.py) are
exported here, resolved on first use so that importing the package stays as cheap as it was."""

_RENDER = ("MeshTable", "render_labels", "vertex_field", "render_ground_truth", "mask_iou")
_MODELS = ("extent", "farthest_points", "diameter", "corners_3d", "keypoints_3d")
__all__ = [*_RENDER, *_MODELS]


def __getattr__(name):
    if name in _RENDER:
        from . import render
        return getattr(render, name)
    if name in _MODELS:
        from . import models
        return getattr(models, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
