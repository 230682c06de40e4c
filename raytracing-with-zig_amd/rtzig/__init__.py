"""rtzig — MI355X-native drop-in for the per-pixel sampling hot path of
AndrewJarrett/raytracing-with-zig (Camera.render, src/camera.zig:123-145).

Product path: C ABI (include/rt.h) -> librtzig.so -> HIP megakernel on gfx950.
"""
from .abi import (OCCLUSION_TARGETS, RT_DIELECTRIC, RT_LAMBERTIAN, RT_METAL, RT_OUT_LINEAR_F64, RT_OUT_RGB8,
                  RtCamera, RtCameraParams, RtDenoiseParams, RtOptions, RtRadianceParams, RtRayHits, RtSphere,
                  RtTemporalFrame, RtTemporalParams)
from .api import (PPM, Camera, CameraBuilder, DeviceRenderer, Scene, chapter9_camera,
                  chapter13_camera, denoise_params, encode_p3, encode_p6, final_scene_camera, occluded,
                  radiance, release_cached_contexts, render, render_adaptive, render_denoised, render_features,
                  render_progressive, render_sequence, sample_key, temporal_params, to_rgb8, trace_rays)
from .lib import EXPORTED, LIB_PATH, RtError, load

__all__ = [
    "OCCLUSION_TARGETS", "RT_DIELECTRIC", "RT_LAMBERTIAN", "RT_METAL", "RT_OUT_LINEAR_F64", "RT_OUT_RGB8",
    "RtCamera", "RtCameraParams", "RtDenoiseParams", "RtOptions", "RtRadianceParams", "RtRayHits", "RtSphere",
    "RtTemporalFrame", "RtTemporalParams",
    "PPM", "Camera", "CameraBuilder", "DeviceRenderer", "Scene", "chapter9_camera",
    "chapter13_camera", "denoise_params", "encode_p3", "encode_p6", "final_scene_camera",
    "release_cached_contexts", "render", "render_adaptive", "render_denoised", "render_features",
    "render_progressive", "render_sequence", "sample_key", "temporal_params", "to_rgb8",
    "trace_rays", "occluded", "radiance",
    "EXPORTED", "LIB_PATH", "RtError", "load",
]
