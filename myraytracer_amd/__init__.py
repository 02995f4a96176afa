"""myraytracer_amd: MI355X-native backend for the per-pixel render loop of
zetanumbers/myraytracer (raytracer/src/shader.wgsl), behind a C ABI.

Importing this package loads myraytracer_amd/lib/libmyraytracer_amd.so and fails loudly
if it has not been built; rendering additionally requires a gfx950 GPU.
"""
from . import _lib
from .api import (DIELECTRIC, LAMBERTIAN, MATERIAL_DTYPE, METAL, SPHERE_DTYPE, Args, Camera, Dielectric, Lambertian, Metal,
                  MrtError, Sphere, State, World, camera_derive, frame_shuffle, frame_weight, pack_world,
                  denoise_mix_default, denoise_params_default, gather, load_scene, material_shade, materials_of, noise_factor, pixel_seed, save_scene, scene_cover, scene_default, scene_stress, shard_global_row,
                  shard_local_rows, srgb8_thresholds, temporal_params_default, temporal_response_default, unshard_rows, view_default, width_policy, width_replay, write_image)

_lib.load()

__all__ = ["Args", "Camera", "Dielectric", "Lambertian", "Metal", "Sphere", "State", "World", "MrtError",
           "LAMBERTIAN", "METAL", "DIELECTRIC", "SPHERE_DTYPE", "MATERIAL_DTYPE", "material_shade", "materials_of", "pack_world", "camera_derive", "frame_weight",
           "frame_shuffle", "pixel_seed", "scene_default", "scene_cover", "scene_stress", "save_scene", "load_scene", "write_image",
           "denoise_mix_default", "denoise_params_default", "gather", "noise_factor", "shard_global_row", "shard_local_rows", "srgb8_thresholds", "temporal_params_default", "temporal_response_default", "unshard_rows", "view_default", "width_policy", "width_replay"]
