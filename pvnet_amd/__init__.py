"""PVNet's inference side on AMD Instinct: see README.md for the modules.

The ground-truth side (pvnet_amd/render.py) is exported here, resolved on first use so that
importing the package stays as cheap as it was."""

_RENDER = ("MeshTable", "render_labels", "vertex_field", "render_ground_truth", "mask_iou")
__all__ = list(_RENDER)


def __getattr__(name):
    if name in _RENDER:
        from . import render
        return getattr(render, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
