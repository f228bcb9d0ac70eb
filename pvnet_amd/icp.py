"""Depth pose refinement on the device: a projective point-to-plane ICP against the sensor's depth map
(include/pvicp.h).  An RGB-only PnP pose has its largest error along the optical axis; on an RGB-D
set (LINEMOD, Occlusion-LINEMOD, YCB-V) this is the step between ``Evaluator.evaluate`` and
``Evaluator.bop_errors`` that removes it.

* :func:`refine_depth` runs the loop: ``render_labels`` renders each pose alone into its own depth
  map, ``pv_icp_iterate`` takes one damped Gauss-Newton step per pose, `iters` times.
* :func:`iterate` is one ``pv_icp_iterate`` call on maps the caller rendered.
* :func:`linearise` returns the normal equations of one call, for inspection.

**Units.**  Depth maps, mesh vertices and the poses' translations share one unit, and ``dist_max``,
``edge_max``, ``max_trans`` and ``eps_trans`` are in it.  The defaults are metres, for LINEMOD-sized
objects (0.1 to 0.3 m across, 0.5 to 1.5 m away); with millimetre meshes (BOP's) scale those four by
1000.  ``max_rot`` and ``eps_rot`` are radians.

No CPU fallback: without libpvicp.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes

import torch

from . import _icp_lib
from .ransac_voting_gpu import VotingWorkspace

# metres and radians: see the module's docstring
DEFAULTS = dict(dist_max=0.02,    # a sensor point farther than this from the rendered one is another surface
                edge_max=0.01,    # a rendered depth step above this is a silhouette or a crease: no normal there
                lam=1e-6,         # Levenberg damping, relative to the diagonal
                min_count=30,     # fewer used pixels than this: leave the pose
                max_rot=0.2,      # the largest step, radians and metres
                max_trans=0.05,
                eps_rot=1e-5,     # a step below both is convergence
                eps_trans=1e-5)
STATUS = _icp_lib.STATUS

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own


def _camera(K, b, dev):
    Kt = torch.as_tensor(K, dtype=torch.float64).to(dev).contiguous()
    if tuple(Kt.shape) == (3, 3):
        return Kt, 0
    if tuple(Kt.shape) == (b, 3, 3):
        return Kt, 9
    raise RuntimeError("K must be [3, 3] or [b, 3, 3]")


def _ids(x, b, dev, name):
    if x is None:
        return None
    t = torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (b,):
        raise RuntimeError(f"{name} must be [b]")
    return t


def _params(kw: dict) -> dict:
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unknown ICP parameter {k!r}: choose from {tuple(DEFAULTS)}")
        p[k] = v
    return p


def new_state(poses: torch.Tensor, neq: bool = False) -> dict:
    """The state a first :func:`iterate` call starts from: a float64 copy of `poses` [b, 3, 4], status
    running, iters 0, and the output tensors (``neq`` only on request)."""
    if not isinstance(poses, torch.Tensor) or poses.device.type != "cuda":
        raise RuntimeError("poses must be a device tensor (no CPU path)")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise RuntimeError("poses must be [b, 3, 4]")
    b, dev = int(poses.shape[0]), poses.device
    st = dict(pose=poses.to(torch.float64).contiguous().clone(),
              status=torch.zeros(b, dtype=torch.int32, device=dev), iters=torch.zeros(b, dtype=torch.int32, device=dev),
              cnt=torch.zeros(b, dtype=torch.int32, device=dev), stats=torch.zeros((b, 3), dtype=torch.float64, device=dev))
    if neq:
        st["neq"] = torch.zeros((b, _icp_lib.PV_ICP_NSUM), dtype=torch.float64, device=dev)
    return st


def iterate(state: dict, depth_est: torch.Tensor, depth: torch.Tensor, K, img_id=None, **kw) -> dict:
    """One ``pv_icp_iterate`` call, in place on `state` (:func:`new_state`): two launches, nothing
    allocated beyond the per-stream workspace's first use, nothing read back.

    depth_est  f32 [b, H, W] contiguous: pose i rendered alone at ``state["pose"][i]``
    depth      f32 [n_img, H, W] contiguous: the sensor's depth, 0 where it is missing
    K          f64 device tensor [3, 3] or [b, 3, 3] (anything else is converted, which allocates)
    img_id     int32 [b] device tensor, or None = image i for pose i
    kw         any of :data:`DEFAULTS`"""
    p = _params(kw)
    pose = state["pose"]
    if not isinstance(pose, torch.Tensor) or pose.device.type != "cuda":
        raise RuntimeError("state['pose'] must be a device tensor (no CPU path)")
    dev, b = pose.device, int(pose.shape[0])
    if depth_est.device != dev or depth.device != dev:
        raise RuntimeError("the depth maps and the poses must be on the same device")
    if depth_est.dim() != 3 or int(depth_est.shape[0]) != b or depth.dim() != 3 or depth.shape[1:] != depth_est.shape[1:]:
        raise RuntimeError("depth_est must be [b, H, W] and depth [n_img, H, W]")
    if depth_est.dtype != torch.float32 or depth.dtype != torch.float32 or not depth_est.is_contiguous() or \
            not depth.is_contiguous():
        raise RuntimeError("the depth maps must be contiguous float32")
    want = dict(pose=((b, 3, 4), torch.float64), status=((b,), torch.int32), iters=((b,), torch.int32),
                cnt=((b,), torch.int32), stats=((b, 3), torch.float64), neq=((b, _icp_lib.PV_ICP_NSUM), torch.float64))
    for k, (shape, dt) in want.items():
        t = state.get(k)
        if t is None and k == "neq":
            continue
        if not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != shape or t.dtype != dt or \
                not t.is_contiguous():
            raise RuntimeError(f"state[{k!r}] must be a contiguous {dt} tensor of shape {list(shape)} on the poses' device")
    H, W = int(depth_est.shape[1]), int(depth_est.shape[2])
    Kt, ks = _camera(K, b, dev)
    iid = _ids(img_id, b, dev, "img_id")
    L = _icp_lib.load()
    need = int(L.pv_icp_workspace_size(b, H, W))
    ws = _ws.get(dev, max(need, 256))
    bt = _icp_lib.IcpBatch(b, int(depth.shape[0]), H, W, int(p["min_count"]), 0, depth.data_ptr(),
                           None if iid is None else iid.data_ptr(), depth_est.data_ptr(), Kt.data_ptr(), ks,
                           float(p["dist_max"]), float(p["edge_max"]), float(p["lam"]), float(p["max_rot"]),
                           float(p["max_trans"]), float(p["eps_rot"]), float(p["eps_trans"]))
    neq = state.get("neq")
    so = _icp_lib.IcpState(pose.data_ptr(), state["status"].data_ptr(), state["iters"].data_ptr(), state["cnt"].data_ptr(),
                           state["stats"].data_ptr(), None if neq is None else neq.data_ptr())
    with torch.cuda.device(dev):
        _icp_lib.check(L.pv_icp_iterate(ctypes.byref(bt), ctypes.byref(so), ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream), "pv_icp_iterate")
    return state


def _render(table, pose, mid, Kc, H, W, znear, out):
    from .render import render_labels
    return render_labels(table, pose[:, None], mid[:, None], None, Kc, H, W, znear=znear, want=("depth",),
                         out={"depth": out})["depth"]


def _prepare(table, poses, model_id, depth, K, img_id):
    if not isinstance(poses, torch.Tensor) or poses.device.type != "cuda":
        raise RuntimeError("poses must be a device tensor (no CPU path)")
    dev = poses.device
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise RuntimeError("poses must be [b, 3, 4]")
    if not isinstance(depth, torch.Tensor) or depth.device != dev or depth.dim() != 3:
        raise RuntimeError("depth must be an [n_img, H, W] tensor on the poses' device")
    b = int(poses.shape[0])
    Kt, ks = _camera(K, b, dev)
    mid = torch.zeros(b, dtype=torch.int32, device=dev) if model_id is None else _ids(model_id, b, dev, "model_id")
    iid = torch.arange(b, dtype=torch.int32, device=dev) if img_id is None else _ids(img_id, b, dev, "img_id")
    return dev, b, Kt, ks, mid, iid, depth.to(torch.float32).contiguous()


def refine_depth(table, poses: torch.Tensor, model_id, depth: torch.Tensor, K, img_id=None, iters: int = 8,
                 znear: float = 1e-3, max_frames: int = 64, **kw):
    """Refine a batch of poses against the sensor's depth.

    table     :class:`~pvnet_amd.render.MeshTable`
    poses     [b, 3, 4] device tensor (any float dtype; the result is float64)
    model_id  int [b], or None = model 0
    depth     f32 [n_img, H, W] device tensor: the sensor's depth, 0 (or anything not finite and > 0)
              where it is missing, in the units of the meshes and the translations
    K         [3, 3] shared or [b, 3, 3]
    img_id    int [b]: the sensor image of each pose; None = image i for pose i
    iters     render + step rounds; a pose that converges earlier is left alone from then on
    kw        any of :data:`DEFAULTS` (``dist_max``, ``edge_max``, ``lam``, ``min_count``, ``max_rot``,
              ``max_trans``, ``eps_rot``, ``eps_trans``): metres and radians by default

    The poses are worked through in chunks of `max_frames` (one rendered depth map per pose is kept
    for a chunk).  The rendered maps and the workspace are allocated once per chunk, before the loop.

    Returns ``(poses f64 [b, 3, 4], info)`` with info = {"status" i32 [b] (``_icp_lib.PV_ICP_*``;
    :data:`STATUS` names them), "iters" i32 [b]: steps taken, "cnt" i32 [b]: pixels used by the last
    step, "rms" f64 [b]: the point-to-plane RMS before the last step, "step" f64 [b, 2]: the last
    step's rotation and translation norms}.  Nothing is read back and nothing synchronises."""
    _params(kw)
    dev, b, Kt, ks, mid, iid, dt = _prepare(table, poses, model_id, depth, K, img_id)
    if int(max_frames) < 1 or int(iters) < 0:
        raise RuntimeError("max_frames must be at least 1 and iters at least 0")
    H, W = int(dt.shape[1]), int(dt.shape[2])
    st = new_state(poses)
    for lo in range(0, b, int(max_frames)):
        hi = min(b, lo + int(max_frames))
        part = {k: v[lo:hi] for k, v in st.items()}
        Kc = Kt if ks == 0 else Kt[lo:hi]
        buf = torch.empty((hi - lo, H, W), dtype=torch.float32, device=dev)
        for _ in range(int(iters)):
            _render(table, part["pose"], mid[lo:hi], Kc, H, W, znear, buf)
            iterate(part, buf, dt, Kc, iid[lo:hi], **kw)
    info = dict(status=st["status"], iters=st["iters"], cnt=st["cnt"], rms=st["stats"][:, 0], step=st["stats"][:, 1:])
    return st["pose"], info


def linearise(table, poses: torch.Tensor, model_id, depth: torch.Tensor, K, img_id=None, znear: float = 1e-3, **kw) -> dict:
    """The normal equations of one step at `poses`, which are not changed: renders, makes one
    ``pv_icp_iterate`` call on a copy and returns {"neq" f64 [b, 28]: A's upper triangle row by row
    (21), g (6), E (1), before damping; "cnt" i32 [b]; "status" i32 [b]; "stats" f64 [b, 3]; "pose":
    where that one step leads; "depth_est" f32 [b, H, W]: the rendered maps}."""
    _params(kw)
    dev, b, Kt, ks, mid, iid, dt = _prepare(table, poses, model_id, depth, K, img_id)
    H, W = int(dt.shape[1]), int(dt.shape[2])
    st = new_state(poses, neq=True)
    buf = torch.empty((b, H, W), dtype=torch.float32, device=dev)
    if b:
        _render(table, st["pose"], mid, Kt, H, W, znear, buf)
        iterate(st, buf, dt, Kt, iid, **kw)
    return dict(neq=st["neq"], cnt=st["cnt"], status=st["status"], stats=st["stats"], pose=st["pose"], depth_est=buf)
