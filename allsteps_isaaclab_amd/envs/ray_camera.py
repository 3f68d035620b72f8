"""The host side of ``cfg.camera``: a ``RayCasterCameraCfg`` (or a dict of up to four named ones) checked against what
the device kernel serves and turned into the call's constants, the intrinsic matrix, the pixels' local directions and
the offset in the "world" camera convention (no device needed).  ``views._RayCasterCamera`` holds the device buffers.

The reference's camera casts against one static warp mesh; here the surfaces are the ground plane and the env's
stones, closed-form in ``k_ray_camera`` (csrc/allsteps_ray_camera.h), so ``mesh_prim_paths`` may name either or both,
as for the height scanner.  Everything the kernel does not serve is refused here with a ``NativeError`` that names
the field.
"""

from __future__ import annotations

import math
import re

import numpy as np
import torch

from .. import _native
from .ray_caster import GROUND_PATH, GROUND_Z, STONES_PATH

DEFAULT_NAME = "camera"  # the name of the single-cfg form
MAX_CAMERAS = 4
DATA_TYPES = ("distance_to_image_plane", "distance_to_camera", "normals")
# ray_caster_camera.py:49-64
UNSUPPORTED_TYPES = {
    "rgb", "instance_id_segmentation", "instance_id_segmentation_fast", "instance_segmentation",
    "instance_segmentation_fast", "semantic_segmentation", "skeleton_data", "motion_vectors", "bounding_box_2d_tight",
    "bounding_box_2d_tight_fast", "bounding_box_2d_loose", "bounding_box_2d_loose_fast", "bounding_box_3d",
    "bounding_box_3d_fast",
}
CLIPPING = {"none": _native.CAM_CLIP_NONE, "max": _native.CAM_CLIP_MAX, "zero": _native.CAM_CLIP_ZERO}

# A camera frame in the "ros" (forward +Z, up -Y) or "opengl" (forward -Z, up +Y) convention, seen from the "world"
# convention (forward +X, up +Z): q_world = q_convention x TO_WORLD[convention], a fixed quarter-turn composition
# whose components are all +-1/2; the way back is the conjugate.  ("world": used as given.)
TO_WORLD = {"ros": (0.5, 0.5, -0.5, 0.5), "opengl": (0.5, -0.5, 0.5, 0.5)}
CONVENTIONS = ("opengl", "ros", "world")


def quat_product(a, b):
    """The product of (w, x, y, z) quaternions given as sequences of four components (floats or tensors), in the
    form and order of csrc/allsteps_imu.h's imu_quat_mul (math.py:489-497)."""
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = (ww + yy) + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return ((qq - ww) + (z1 - y1) * (y2 - z2), (qq - xx) + (x1 + w1) * (x2 + w2),
            (qq - yy) + (w1 - x1) * (y2 + z2), (qq - zz) + (z1 + y1) * (w2 - x2))


def offset_quat_to_world(rot, convention: str) -> tuple:
    """``convert_camera_frame_orientation_convention(rot, origin=convention, target="world")`` (math.py:1429-1509) of
    one quaternion in Python floats: "world" is returned as given; the others go through rotation matrices in the
    reference, which yields the unit quaternion of the composed rotation -- here the product with the fixed
    quaternion, normalised.  Equal to the reference's up to the sign of the quaternion."""
    rot = tuple(float(x) for x in rot)
    if convention == "world":
        return rot
    q = quat_product(rot, TO_WORLD[convention])
    nrm = math.sqrt(sum(x * x for x in q))
    return tuple(x / nrm for x in q)


def quat_to_world_torch(q: torch.Tensor, convention: str) -> torch.Tensor:
    """``offset_quat_to_world`` of (k, 4) device quaternions, in torch."""
    if convention == "world":
        return q.clone()
    out = torch.stack(quat_product(q.unbind(-1), TO_WORLD[convention]), -1)
    return out / out.norm(dim=-1, keepdim=True)


def quat_from_world_torch(q: torch.Tensor, convention: str) -> torch.Tensor:
    """(k, 4) "world"-convention quaternions in ``convention`` (``data.quat_w_ros`` / ``quat_w_opengl``)."""
    if convention == "world":
        return q.clone()
    w, x, y, z = TO_WORLD[convention]
    out = torch.stack(quat_product(q.unbind(-1), (w, -x, -y, -z)), -1)
    return out / out.norm(dim=-1, keepdim=True)


def world_pose_offsets(root_pos: torch.Tensor, root_quat: torch.Tensor, positions, orientations, convention: str):
    """``RayCasterCamera.set_world_poses`` (ray_caster_camera.py:186-201) for k envs, in torch on the tensors' device:
    the offsets (position (k, 3) or None, "world"-convention quaternion (k, 4) or None) that put the cameras at
    ``positions`` (k, 3) with ``orientations`` (k, 4) given in ``convention``, against the view poses ``root_pos``
    (k, 3) and ``root_quat`` (k, 4)."""
    from .ray_caster import quat_apply

    if convention not in CONVENTIONS:
        raise ValueError(f"convention {convention!r} is not 'opengl', 'ros' or 'world'")
    conj = root_quat * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=root_quat.dtype, device=root_quat.device)
    q_inv = conj / root_quat.norm(dim=-1, keepdim=True).clamp(min=1e-9)
    off_pos = off_quat = None
    if positions is not None:
        off_pos = quat_apply(q_inv, positions.reshape(-1, 3) - root_pos)
    if orientations is not None:
        q_set = quat_to_world_torch(orientations.reshape(-1, 4), convention)
        off_quat = torch.stack(quat_product(q_inv.unbind(-1), q_set.unbind(-1)), -1)
    return off_pos, off_quat


def intrinsic_matrix(pattern) -> np.ndarray:
    """``RayCasterCamera._compute_intrinsic_matrices`` (ray_caster_camera.py:370-392) in Python floats, stored to
    float32 (3, 3).  Like the reference it fills in ``pattern.vertical_aperture`` when that is None."""
    if pattern.vertical_aperture is None:
        pattern.vertical_aperture = pattern.horizontal_aperture * pattern.height / pattern.width
    f_x = pattern.width * pattern.focal_length / pattern.horizontal_aperture
    f_y = pattern.height * pattern.focal_length / pattern.vertical_aperture
    c_x = pattern.horizontal_aperture_offset * f_x + pattern.width / 2
    c_y = pattern.vertical_aperture_offset * f_y + pattern.height / 2
    k = np.zeros((3, 3), np.float32)
    k[0, 0], k[0, 2], k[1, 1], k[1, 2], k[2, 2] = f_x, c_x, f_y, c_y, 1.0
    return k


def named_cfgs(cfg) -> dict:
    """``cfg.camera`` as a dict name -> RayCasterCameraCfg: a single cfg is registered as ``"camera"``."""
    if isinstance(cfg, dict):
        if not cfg:
            raise _native.NativeError("cfg.camera: an empty dict names no sensor; use None for no camera")
        for name in cfg:
            if not isinstance(name, str) or not name:
                raise _native.NativeError(f"cfg.camera: the key {name!r} is not a sensor name")
        if len(cfg) > MAX_CAMERAS:
            raise _native.NativeError(f"cfg.camera: {len(cfg)} cameras; at most {MAX_CAMERAS} are served (each has "
                                      f"its own buffers and its own launch of the HIP kernel)")
        return dict(cfg)
    return {DEFAULT_NAME: cfg}


class RayCameraSpec:
    """A checked ``RayCasterCameraCfg``: ``surfaces`` (AS_RAY_* bits), ``clipping`` (AS_CAM_CLIP_*), ``width``,
    ``height``, ``num_rays``, ``max_distance``, ``data_types``, ``intrinsics`` float32 (3, 3), ``dirs`` float32 (3, R)
    -- the pixels' local directions, pixel (row v, column u) at ``v * width + u`` -- and ``offset`` float32 (7,),
    position | quaternion (w, x, y, z) in the "world" convention."""

    def __init__(self, cfg, *, root_body: str, step_dt: float, step_paths=(), name: str = DEFAULT_NAME):
        self.cfg, self.name = cfg, name
        where = "cfg.camera" if name == DEFAULT_NAME else f"cfg.camera[{name!r}]"

        def refuse(field: str, detail: str) -> "_native.NativeError":
            return _native.NativeError(f"{where}.{field}: {detail}.  The images are cast by a HIP kernel against the "
                                       f"ground plane and the stones (no host fallback)")

        self._refuse = refuse
        # RayCasterCamera._check_supported_data_types (ray_caster_camera.py:331-342), the reference's own refusal
        types = getattr(cfg, "data_types", None)
        if not isinstance(types, (list, tuple)) or len(types) == 0 or not all(isinstance(t, str) for t in types):
            raise refuse("data_types", f"{types!r} is not a non-empty list of data type names")
        common = set(types) & UNSUPPORTED_TYPES
        if common:
            raise ValueError(f"RayCasterCamera class does not support the following sensor types: {common}."
                             "\n\tThis is because these sensor types cannot be obtained in a fast way using ''warp''."
                             "\n\tHint: If you need to work with these sensor types, we recommend using the USD camera"
                             " interface from the isaaclab.sensors.camera module.")
        for t in types:  # _create_buffers (:360-366)
            if t not in DATA_TYPES:
                raise ValueError(f"Received unknown data type: {t}. Please check the configuration.")
        self.data_types = list(dict.fromkeys(types))
        path = getattr(cfg, "prim_path", None)
        if not isinstance(path, str) or not path:
            raise refuse("prim_path", f"{path!r} is not a prim path")
        leaf = path.split("/")[-1]
        if re.match(r"^[a-zA-Z0-9/_]+$", leaf) is None:  # the reference's own refusal (ray_caster.py:61-67)
            raise RuntimeError(f"Invalid prim path for the ray-caster sensor: {path}."
                               "\n\tHint: Please ensure that the prim path does not contain any regex patterns in the "
                               "leaf.")
        if leaf != root_body:
            raise refuse("prim_path", f"{path!r} attaches the camera to {leaf!r}; only the robot's root body "
                                      f"{root_body!r} is served (its pose is the state's root_pos / root_quat)")
        meshes = getattr(cfg, "mesh_prim_paths", None)
        if not isinstance(meshes, (list, tuple)) or len(meshes) == 0:
            raise refuse("mesh_prim_paths", f"{meshes!r} is not a non-empty list of prim paths")
        stones = {STONES_PATH, *step_paths}
        self.surfaces = 0
        for m in meshes:
            if m == GROUND_PATH:
                self.surfaces |= _native.RAY_GROUND
            elif m in stones:
                self.surfaces |= _native.RAY_STONES  # any of the stones' paths selects all of the env's stones
            else:
                raise refuse("mesh_prim_paths", f"{m!r} is neither the ground plane {GROUND_PATH!r} nor the stones "
                                                f"({STONES_PATH!r} or an entry of cfg.step_paths)")
        clip = getattr(cfg, "depth_clipping_behavior", "none")
        if clip not in CLIPPING:
            raise refuse("depth_clipping_behavior", f"{clip!r} is not 'max', 'zero' or 'none'")
        self.clipping = CLIPPING[clip]
        drift = tuple(getattr(cfg, "drift_range", (0.0, 0.0)))
        if len(drift) != 2 or any(float(x) != 0.0 for x in drift):
            raise refuse("drift_range", f"{drift!r} is not (0.0, 0.0): the camera draws nothing")
        period = float(getattr(cfg, "update_period", 0.0))
        if not period <= step_dt:
            raise refuse("update_period", f"{period!r} s is longer than the env step ({step_dt!r} s): the images would "
                                          f"have to go stale across steps, and the sensor keeps no timestamp")
        if getattr(cfg, "history_length", 0) != 0:
            raise refuse("history_length", f"{cfg.history_length!r} is not 0: the camera keeps the last image only")
        if getattr(cfg, "debug_vis", False):
            raise refuse("debug_vis", "True asks for visualization markers, which a headless env has not")
        self.max_distance = float(getattr(cfg, "max_distance", 1e6))
        if not math.isfinite(self.max_distance) or self.max_distance <= 0.0:
            raise refuse("max_distance", f"{self.max_distance!r} is not a finite positive distance")
        offset = getattr(cfg, "offset", None)
        convention = getattr(offset, "convention", "ros")
        if convention not in CONVENTIONS:
            raise refuse("offset.convention", f"{convention!r} is not 'opengl', 'ros' or 'world'")
        pos, rot = list(getattr(offset, "pos", ())), list(getattr(offset, "rot", ()))
        if len(pos) != 3 or len(rot) != 4 or not all(math.isfinite(float(x)) for x in pos + rot) \
                or not any(float(x) != 0.0 for x in rot):
            raise refuse("offset", f"pos {pos!r} / rot {rot!r} is not a finite position and a non-zero quaternion")
        self.convention = convention
        self.offset = np.asarray([*pos, *offset_quat_to_world(rot, convention)], np.float32)

        from ..utils.patterns import PinholeCameraPatternCfg

        pattern = getattr(cfg, "pattern_cfg", None)
        if not isinstance(pattern, PinholeCameraPatternCfg) or not callable(getattr(pattern, "func", None)):
            raise refuse("pattern_cfg", f"{pattern!r} is not a PinholeCameraPatternCfg with a func(cfg, intrinsic_"
                                        f"matrices, device)")
        for side in ("width", "height"):
            v = getattr(pattern, side)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise refuse("pattern_cfg", f"{side} {v!r} is not a positive int")
        self.pattern = pattern
        self.width, self.height = pattern.width, pattern.height
        self.num_rays = self.width * self.height
        if self.num_rays > _native.MAX_CAMERA_RAYS:
            raise refuse("pattern_cfg", f"{self.height} x {self.width} = {self.num_rays} pixels; the kernel takes at "
                                        f"most AS_MAX_CAMERA_RAYS = {_native.MAX_CAMERA_RAYS}")
        for k in ("focal_length", "horizontal_aperture", "vertical_aperture", "horizontal_aperture_offset",
                  "vertical_aperture_offset"):
            v = getattr(pattern, k)
            if not (v is None and k == "vertical_aperture") and not (isinstance(v, (int, float))
                                                                     and math.isfinite(v)):
                raise refuse("pattern_cfg", f"{k} {v!r} is not a finite number")
        if not pattern.focal_length > 0 or not pattern.horizontal_aperture > 0 \
                or not (pattern.vertical_aperture is None or pattern.vertical_aperture > 0):
            raise refuse("pattern_cfg", "focal_length and the apertures must be positive")
        self.intrinsics = intrinsic_matrix(pattern)
        self.dirs = self.directions(self.intrinsics)

    def directions(self, intrinsics) -> np.ndarray:
        """float32 (3, R): the pattern's local directions for one (3, 3) intrinsic matrix; its starts must be zero
        (the kernel casts every ray from the camera's position)."""
        k = torch.as_tensor(np.asarray(intrinsics, np.float32)).reshape(1, 3, 3)
        starts, directions = self.pattern.func(self.pattern, k, "cpu")
        starts, directions = torch.as_tensor(starts), torch.as_tensor(directions)
        if directions.shape != (1, self.num_rays, 3) or starts.shape != directions.shape:
            raise self._refuse("pattern_cfg", f"func returned shapes {tuple(starts.shape)} and "
                                              f"{tuple(directions.shape)}, not (1, {self.num_rays}, 3) twice")
        if bool((starts != 0).any()):
            raise self._refuse("pattern_cfg", "func returned ray starts that are not all zero: a pinhole camera casts "
                                              "every ray from its optical centre")
        dirs = np.ascontiguousarray(directions[0].to(torch.float32).numpy().T)
        if not np.isfinite(dirs).all():
            raise self._refuse("pattern_cfg", "a ray direction is not finite in float32")
        return dirs

    def native_cfg(self) -> "_native.AsRayCamera":
        c = _native.AsRayCamera()
        c.width, c.height, c.surfaces, c.clipping = self.width, self.height, self.surfaces, self.clipping
        c.max_distance, c.ground_z = self.max_distance, GROUND_Z
        return c

    def surface_names(self) -> list:
        return [name for bit, name in ((_native.RAY_GROUND, "ground"), (_native.RAY_STONES, "stones"))
                if self.surfaces & bit]
