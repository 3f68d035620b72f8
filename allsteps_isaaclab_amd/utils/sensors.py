"""Sensor configuration -- ``RayCasterCfg``, ``RayCasterCameraCfg``, ``patterns``, ``ImuCfg``,
``FrameTransformerCfg`` and ``OffsetCfg`` of ``isaaclab.sensors`` and the observation functions ``height_scan``,
``image``, ``imu_orientation``, ``imu_ang_vel`` and ``imu_lin_acc`` of ``isaaclab.envs.mdp``, same names, fields and
defaults, for ``cfg.height_scanner``, ``cfg.camera``, ``cfg.imu`` and ``cfg.frame_transformer`` of the envs.

The rays are cast on the device (``k_ray_cast``, csrc/ray_caster_kernels.h; the camera's by ``k_ray_camera``,
csrc/ray_camera_kernels.h) against the ground plane and the env's stones, and the IMUs are updated on the device
(``k_imu``, csrc/imu_kernels.h), as are the frame transformers (``k_frame_transformer``,
csrc/frame_transformer_kernels.h); the env raises at construction for what those kernels do not serve
(envs/ray_caster.py, envs/ray_camera.py, envs/imu.py, envs/frame_transformer.py).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any

from . import patterns  # noqa: F401  (isaaclab.sensors.patterns)
from .events import SceneEntityCfg
from .noise import MISSING


@dataclass
class RayCasterCfg:
    """ray_caster_cfg.py ``RayCasterCfg`` with ``SensorBaseCfg``'s fields (sensor_base_cfg.py)."""

    @dataclass
    class OffsetCfg:
        """The sensor frame's pose in the frame of the body it is attached to."""

        pos: tuple = (0.0, 0.0, 0.0)
        rot: tuple = (1.0, 0.0, 0.0, 0.0)  # (w, x, y, z)

    prim_path: str = MISSING
    update_period: float = 0.0
    history_length: int = 0
    debug_vis: bool = False
    mesh_prim_paths: Any = MISSING  # list[str]
    offset: OffsetCfg = field(default_factory=OffsetCfg)
    attach_yaw_only: bool = MISSING
    pattern_cfg: Any = MISSING  # a patterns.PatternBaseCfg
    max_distance: float = 1e6
    drift_range: tuple = (0.0, 0.0)


def height_scan(env, sensor_cfg, offset: float = 0.5):
    """observations.py ``height_scan``: the sensor's height over every hit point, less ``offset`` -- (N, R)."""
    sensor = env.scene.sensors[sensor_cfg.name]
    return sensor.data.pos_w[:, 2].unsqueeze(1) - sensor.data.ray_hits_w[..., 2] - offset


@dataclass
class RayCasterCameraCfg(RayCasterCfg):
    """ray_caster_camera_cfg.py ``RayCasterCameraCfg``: a depth camera on the ray caster's cast."""

    @dataclass
    class OffsetCfg:
        """The camera frame's pose in the frame of the body it is attached to, ``rot`` in ``convention``: "opengl"
        (forward -Z, up +Y), "ros" (forward +Z, up -Y) or "world" (forward +X, up +Z)."""

        pos: tuple = (0.0, 0.0, 0.0)
        rot: tuple = (1.0, 0.0, 0.0, 0.0)  # (w, x, y, z)
        convention: str = "ros"

    offset: OffsetCfg = field(default_factory=OffsetCfg)
    data_types: list = field(default_factory=lambda: ["distance_to_image_plane"])
    depth_clipping_behavior: str = "none"  # "max" | "zero" | "none"
    pattern_cfg: Any = MISSING  # a patterns.PinholeCameraPatternCfg

    def __post_init__(self):
        self.attach_yaw_only = False  # a camera always turns with the full orientation


def image(env, sensor_cfg: SceneEntityCfg = SceneEntityCfg("tiled_camera"), data_type: str = "rgb",
          convert_perspective_to_orthogonal: bool = False, normalize: bool = True):
    """observations.py ``image``: the camera's images of ``data_type`` -- (N, H, W, C), a clone.  With ``normalize``
    the depth types get their infinite values replaced by zero, in place on the sensor's buffer as in the reference.
    The ray-cast camera renders no colour, and the orthogonal conversion of a perspective depth is not served."""
    if data_type == "rgb":
        raise ValueError("mdp.image: data_type 'rgb' is not served: the ray-cast camera has the data types "
                         "distance_to_image_plane, distance_to_camera and normals")
    if convert_perspective_to_orthogonal:
        raise NotImplementedError("mdp.image: convert_perspective_to_orthogonal=True is not served; ask the camera for "
                                  "distance_to_image_plane, which is the orthogonal depth")
    sensor = env.scene.sensors[sensor_cfg.name]
    images = sensor.data.output[data_type]
    if normalize and ("distance_to" in data_type or "depth" in data_type):
        images[images == float("inf")] = 0
    return images.clone()


@dataclass
class ImuCfg:
    """imu_cfg.py ``ImuCfg`` with ``SensorBaseCfg``'s fields (sensor_base_cfg.py); ``visualizer_cfg`` serves
    ``debug_vis`` only, which a headless env refuses."""

    @dataclass
    class OffsetCfg:
        """The sensor frame's pose in the frame of the body it is attached to."""

        pos: tuple = (0.0, 0.0, 0.0)
        rot: tuple = (1.0, 0.0, 0.0, 0.0)  # (w, x, y, z)

    prim_path: str = MISSING
    update_period: float = 0.0
    history_length: int = 0
    debug_vis: bool = False
    offset: OffsetCfg = field(default_factory=OffsetCfg)
    visualizer_cfg: Any = None
    gravity_bias: tuple = (0.0, 0.0, 9.81)


def imu_orientation(env, asset_cfg: SceneEntityCfg = SceneEntityCfg("imu")):
    """observations.py ``imu_orientation``: the sensor's orientation in the world frame, (w, x, y, z) -- (N, 4)."""
    return env.scene[asset_cfg.name].data.quat_w


def imu_ang_vel(env, asset_cfg: SceneEntityCfg = SceneEntityCfg("imu")):
    """observations.py ``imu_ang_vel``: the angular velocity (rad/s) in the sensor frame -- (N, 3)."""
    return env.scene[asset_cfg.name].data.ang_vel_b


def imu_lin_acc(env, asset_cfg: SceneEntityCfg = SceneEntityCfg("imu")):
    """observations.py ``imu_lin_acc``: the linear acceleration (m/s^2) in the sensor frame -- (N, 3)."""
    return env.scene[asset_cfg.name].data.lin_acc_b


@dataclass
class OffsetCfg:
    """frame_transformer_cfg.py ``OffsetCfg``: the offset pose of one frame relative to another frame."""

    pos: tuple = (0.0, 0.0, 0.0)
    rot: tuple = (1.0, 0.0, 0.0, 0.0)  # (w, x, y, z)


@dataclass
class FrameTransformerCfg:
    """frame_transformer_cfg.py ``FrameTransformerCfg`` with ``SensorBaseCfg``'s fields (sensor_base_cfg.py);
    ``visualizer_cfg`` serves ``debug_vis`` only, which a headless env refuses."""

    @dataclass
    class FrameCfg:
        """Information specific to a coordinate frame: the body (a regex may match several), the frame's name
        (None: the body's) and its pose in the body's frame."""

        prim_path: str = MISSING
        name: Any = None  # str | None
        offset: OffsetCfg = field(default_factory=OffsetCfg)

    prim_path: str = MISSING
    update_period: float = 0.0
    history_length: int = 0
    debug_vis: bool = False
    source_frame_offset: OffsetCfg = field(default_factory=OffsetCfg)
    target_frames: Any = MISSING  # list[FrameCfg]
    visualizer_cfg: Any = None
