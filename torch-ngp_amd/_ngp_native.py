"""Loader for libngp_hip.so, the gfx950 C-ABI library behind every op package.

The reference packages bind their CUDA sources through pybind11 (AOT
`_gridencoder`/`_raymarching`/... or JIT `backend.py`, e.g.
gridencoder/backend.py:31-38). Here a single prebuilt shared library exports
the C functions declared in include/ngp_hip.h and each package's backend.py
binds them with ctypes. There is deliberately NO fallback: if the library or
a GPU is missing, every op raises.
"""
import ctypes
import os

import torch  # noqa: F401  (must load libamdhip64 before the library below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NGP_HIP_LIB", os.path.join(_HERE, "libngp_hip.so"))

c_u32 = ctypes.c_uint32
c_i32 = ctypes.c_int32
c_f32 = ctypes.c_float
c_vp = ctypes.c_void_p
c_sz = ctypes.c_size_t

# name -> argtypes (restype int unless listed in _RESTYPES). Mirrors ngp_hip.h.
SIGNATURES = {
    "ngp_abi_version": [],
    "ngp_last_error": [],
    "ngp_grid_encode_forward": [c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_f32, c_u32,
                                c_vp, c_u32, c_i32, c_u32, c_i32, c_i32, c_vp],
    "ngp_grid_encode_backward": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_f32,
                                 c_u32, c_vp, c_vp, c_u32, c_i32, c_u32, c_i32, c_i32, c_vp],
    "ngp_grad_total_variation": [c_vp, c_vp, c_vp, c_vp, c_f32, c_u32, c_u32, c_u32, c_u32, c_f32,
                                 c_u32, c_u32, c_i32, c_i32, c_vp],
    "ngp_near_far_from_aabb": [c_vp, c_vp, c_vp, c_u32, c_f32, c_vp, c_vp, c_vp],
    "ngp_sph_from_ray": [c_vp, c_vp, c_f32, c_u32, c_vp, c_vp],
    "ngp_morton3D": [c_vp, c_u32, c_vp, c_vp],
    "ngp_morton3D_invert": [c_vp, c_u32, c_vp, c_vp],
    "ngp_packbits": [c_vp, c_u32, c_f32, c_vp, c_vp],
    "ngp_march_rays_train_workspace_bytes": [c_u32, c_u32, c_u32, c_u32],
    "ngp_march_rays_train_error_offset": [c_u32, c_u32, c_u32, c_u32],
    "ngp_march_occupancy_build": [c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_sz, c_vp],
    "ngp_march_rays_train_prebuilt": [c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32, c_u32, c_u32,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp],
    "ngp_march_rays_train_prebuilt_tail": [c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32, c_u32, c_u32,
                                           c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz,
                                           c_vp, c_f32, c_f32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp],
    "ngp_march_rays_train_prebuilt_adam": [c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32, c_u32, c_u32,
                                           c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz,
                                           c_vp, c_f32, c_f32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp],
    "ngp_grid_encode_backward_fused_reduce_batch": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32,
                                                    c_u32, c_f32, c_u32, c_u32, c_i32, c_u32, c_vp, c_vp, c_sz,
                                                    c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                    c_vp, c_vp],
    "ngp_grid_encode_backward_fused_reduce_batch_live": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_vp,
                                                         c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_i32, c_u32,
                                                         c_vp, c_vp, c_sz, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                                         c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_march_rays_train": [c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32, c_u32, c_u32,
                             c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp],
    "ngp_composite_rays_train_forward": [c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_vp, c_vp,
                                         c_vp, c_vp],
    "ngp_composite_rays_train_backward": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_vp, c_u32, c_u32, c_f32, c_vp, c_vp, c_vp],
    "ngp_distortion_rays_train_forward": [c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_vp, c_vp],
    "ngp_distortion_rays_train_backward": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_vp, c_vp],
    "ngp_march_rays": [c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32,
                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_grid_encode_forward_fused_tail": [c_vp, c_f32, c_vp, c_i32, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32,
                                           c_f32, c_u32, c_u32, c_i32, c_u32, c_vp, c_f32, c_f32, c_i32, c_i32, c_vp,
                                           c_u32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_render_state_bytes": [],
    "ngp_render_count": [c_vp, c_u32],
    "ngp_render_init": [c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_render_march": [c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_u32, c_u32, c_u32, c_vp,
                         c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_render_composite": [c_u32, c_u32, c_u32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                             c_vp, c_vp],
    "ngp_composite_rays": [c_u32, c_u32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                           c_vp],
    "ngp_sh_encode_forward": [c_vp, c_vp, c_u32, c_u32, c_u32, c_vp, c_i32, c_vp],
    "ngp_sh_encode_backward": [c_vp, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_i32, c_vp],
    "ngp_freq_encode_forward": [c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp],
    "ngp_freq_encode_backward": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp],
    "ngp_ffmlp_forward": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp,
                          c_vp],
    "ngp_ffmlp_inference": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32, c_vp,
                            c_vp, c_vp],
    "ngp_ffmlp_backward_workspace_bytes": [c_u32, c_u32, c_u32, c_u32, c_u32],
    "ngp_ffmlp_backward": [c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32,
                           c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp],
    "ngp_ffmlp_allocate_splitk": [c_sz],
    "ngp_ffmlp_free_splitk": [],
    "ngp_adam_step": [c_vp, c_vp, c_i32, c_vp, c_vp, c_sz, c_f32, c_f32, c_f32, c_f32, c_f32,
                      c_i32, c_f32, c_vp],
    "ngp_grid_encode_forward_fused": [c_vp, c_f32, c_vp, c_i32, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32,
                                      c_u32, c_f32, c_u32, c_u32, c_i32, c_u32, c_i32, c_vp],
    "ngp_grid_encode_backward_fused_workspace_bytes": [c_u32, c_u32, c_u32, c_u32, c_f32, c_u32, c_i32,
                                                       c_vp],
    "ngp_grid_encode_backward_fused": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32,
                                       c_u32, c_f32, c_u32, c_u32, c_i32, c_u32, c_vp, c_vp, c_sz, c_i32,
                                       c_vp, c_vp],
    "ngp_ffmlp_image_bytes": [c_u32, c_u32, c_u32],
    "ngp_grad_guard": [c_vp, ctypes.c_uint64, ctypes.c_uint64, c_i32, c_vp, c_vp],
    "ngp_fused_inf_flag": [c_vp, c_i32],
    "ngp_grid_encode_backward_fused_counter_bytes": [c_u32, c_u32, c_u32, c_u32, c_f32, c_u32, c_i32, c_vp],
    "ngp_fused_optimizer_update": [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_f32, c_f32,
                                   c_i32, c_i32, c_f32, c_i32, c_vp, c_vp],
    "ngp_fused_step_head": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_i32, c_vp, c_f32, c_u32, c_vp,
                            c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_i32, c_i32,
                            c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp],
    "ngp_fused_optimizer_update_head": [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_f32, c_f32,
                                        c_i32, c_i32, c_f32, c_i32, c_vp,
                                        c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_i32, c_vp, c_f32, c_u32,
                                        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp],
    "ngp_ffmlp_pack": [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_ffmlp_forward_rows": [c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_u32, c_u32, c_u32,
                               c_vp, c_vp],
    "ngp_nerf_sigma_forward": [c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp,
                               c_f32, c_u32, c_vp],
    "ngp_nerf_forward": [c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp,
                         c_f32, c_vp, c_vp],
    "ngp_ffmlp_backward_rows": [c_vp, c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_u32, c_u32,
                                c_vp, c_vp, c_i32, c_u32, c_vp, c_sz, c_vp],
    "ngp_nerf_backward": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_u32,
                          c_vp, c_sz, c_vp, c_sz, c_vp, c_vp],
    "ngp_nerf_backward_live": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp, c_vp, c_u32, c_u32, c_u32,
                               c_u32, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp],
    "ngp_ffmlp_reduce": [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp],
    "ngp_fused_state_bytes": [],
    "ngp_fused_state_init": [c_vp, c_f32, c_vp],
    "ngp_lego_rays": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_i32, c_vp, c_f32, c_u32,
                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_image_rays": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_f32, c_u32,
                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_error_map_select": [c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp],
    "ngp_error_map_update": [c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_u32, c_vp, c_vp, c_vp, c_vp],
    "ngp_fused_step_head_images": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_f32, c_u32, c_vp,
                                   c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_i32, c_i32,
                                   c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp],
    "ngp_grid_encode_backward_fused_reduce_batch_images": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_vp,
                                                           c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_i32, c_u32,
                                                           c_vp, c_vp, c_sz, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                                           c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_dw_stash_bytes": [c_u32, c_u32, c_u32],
    "ngp_nerf_backward_live_dw": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp, c_vp, c_u32, c_u32, c_u32,
                                  c_u32, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_u32, c_u32, c_vp],
    "ngp_nerf_dw_reduce": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_vp],
    "ngp_grid_encode_backward_fused_dw_batch_live": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_vp,
                                                     c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_i32, c_u32,
                                                     c_vp, c_vp, c_sz, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp,
                                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_vp],
    "ngp_nerf_glue_forward": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_vp],
    "ngp_nerf_glue_backward": [c_vp, c_vp, c_u32, c_vp, c_vp],
    "ngp_nerf_composite_loss": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_composite_loss_live": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                     c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                     c_vp],
    "ngp_nerf_composite_loss_depth": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                      c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_composite_loss_lists": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                      c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_composite_loss_depth_lists": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                            c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_composite_loss_dist": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                     c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_composite_loss_dist_lists": [c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_f32, c_vp,
                                           c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_nerf_backward_join_dw": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_vp, c_u32, c_vp, c_vp, c_vp,
                                  c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_u32,
                                  c_u32, c_vp],
    "ngp_nerf_backward_join_max_rays": [],
    "ngp_fused_optimizer_step": [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_f32, c_f32, c_f32,
                                 c_i32, c_i32, c_f32, c_f32, c_f32, c_i32, c_i32, c_u32, c_vp, c_vp,
                                 c_vp, c_vp, c_vp],
    "ngp_density_grid_points": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_f32, c_vp, c_vp, c_vp],
    "ngp_nerf_density_forward": [c_vp, c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_f32, c_vp, c_vp, c_vp],
    "ngp_density_grid_ema_pack": [c_vp, c_vp, c_u32, c_u32, c_f32, ctypes.c_double, c_vp, c_vp, c_vp],
    "ngp_density_grid_draw_workspace_bytes": [c_u32, c_u32],
    "ngp_density_grid_sort_workspace_bytes": [c_u32, c_u32],
    "ngp_density_grid_points_sorted": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_vp, c_sz,
                                       c_vp, c_vp, c_vp],
    "ngp_density_grid_draw": [c_vp, c_u32, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_sz, c_vp],
    "ngp_density_mean_count": [c_vp, c_vp, c_vp, c_u32, c_u32, c_vp, c_vp],
    "ngp_nerf_density_forward_rows": [c_vp, c_vp, c_u32, c_u32, c_u32, c_f32, c_vp, c_vp],
    "ngp_density_grid_run_max": [c_vp, c_vp, c_u32, c_u32, c_u32, c_u32, c_vp, c_vp],
    "ngp_density_grid_ostat_workspace_bytes": [c_u32, c_u32],
    "ngp_density_grid_draw_sorted": [c_vp, c_u32, c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_vp, c_sz, c_vp, c_sz,
                                     c_vp, c_vp, c_vp],
    "ngp_grid_encode_backward_fused_timing_offset": [c_u32, c_u32, c_u32, c_u32, c_f32, c_u32, c_i32, c_vp],
    "ngp_grad_exchange_bins": [ctypes.c_uint64],
    "ngp_grad_exchange_words": [ctypes.c_uint64, c_u32],
    "ngp_grad_exchange_list": [c_vp, ctypes.c_uint64, c_vp, c_vp, c_u32, c_vp],
    "ngp_grad_exchange_reduce": [c_vp, c_i32, c_u32, c_vp, ctypes.c_uint64, c_vp, c_vp, c_vp, c_vp],
    "ngp_grid_encode_backward_fused_reduce": [c_vp, c_vp, c_f32, c_vp, c_vp, c_u32, c_vp, c_u32, c_u32, c_u32,
                                              c_f32, c_u32, c_u32, c_i32, c_u32, c_vp, c_vp, c_sz, c_i32, c_vp,
                                              c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_mesh_lattice_points": [c_u32, c_u32, c_u32, c_vp, c_u32, c_u32, c_vp, c_vp],
    "ngp_mesh_workspace_bytes": [c_u32, c_u32, c_u32],
    "ngp_mesh_count": [c_vp, c_u32, c_u32, c_u32, c_f32, c_vp, c_sz, c_vp, c_vp],
    "ngp_mesh_emit": [c_vp, c_u32, c_u32, c_u32, c_f32, c_vp, c_vp, c_sz, ctypes.c_uint64, ctypes.c_uint64,
                      c_vp, c_vp, c_vp, c_vp],
    "ngp_mesh_components": [c_vp, ctypes.c_uint64, ctypes.c_uint64, c_vp, c_vp, c_vp],
    "ngp_mesh_clean_workspace_bytes": [ctypes.c_uint64, ctypes.c_uint64],
    "ngp_mesh_clean_count": [c_vp, ctypes.c_uint64, ctypes.c_uint64, c_vp, c_vp, c_u32, c_i32, c_vp, c_sz, c_vp,
                             c_vp],
    "ngp_mesh_clean_emit": [c_vp, c_vp, c_vp, ctypes.c_uint64, ctypes.c_uint64, c_vp, c_sz, ctypes.c_uint64,
                            ctypes.c_uint64, c_vp, c_vp, c_vp, c_vp],
    "ngp_mesh_color_dirs": [c_vp, ctypes.c_uint64, c_vp, c_vp],
    "ngp_mesh_color_finish": [c_vp, c_u32, ctypes.c_uint64, c_i32, c_vp, c_vp],
    "ngp_frame_begin": [c_vp, c_u32, c_u32, c_vp, c_u32, c_u32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_frame_finish": [c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_frame_sse": [c_u32, c_u32, c_vp, c_vp, c_f32, c_vp, c_u32, c_vp, c_vp],
    "ngp_frame_ssim": [c_u32, c_u32, c_vp, c_vp, c_f32, c_vp, c_u32, c_vp, c_vp, c_vp],
    "ngp_ema_update": [c_vp, c_vp, ctypes.c_uint64, c_f32, c_vp],
    "ngp_background_scratch_bytes": [ctypes.c_uint64],
    "ngp_background_forward": [c_vp, c_vp, c_f32, c_u32, c_vp, c_i32, c_vp, c_u32, c_u32, c_f32, c_u32, c_vp, c_u32,
                               c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_background_backward": [c_vp, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, c_f32, c_u32,
                                ctypes.c_uint64, c_vp, c_u32, c_u32, c_u32, c_vp, c_f32, c_f32, c_vp, c_vp, c_vp,
                                c_vp, c_vp],
    "ngp_jpeg_scan_capacity": [c_u32, c_u32, c_u32],
    "ngp_jpeg_workspace_elems": [c_u32, c_u32, c_u32],
    "ngp_jpeg_encode": [c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp],
    "ngp_sdf_sample": [c_vp, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp],
    "ngp_sdf_query": [c_vp, c_u32, c_vp, c_vp, c_vp, c_u32, c_vp, c_i32, c_vp, c_vp, c_vp],
    "ngp_sdf_mape": [c_vp, c_i32, c_vp, ctypes.c_uint64, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_vm_forward": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp],
    "ngp_vm_grad_values": [c_u32, c_u32, c_u32, c_vp, c_vp],
    "ngp_vm_backward_scratch_bytes": [c_u32, c_u32, c_u32, c_vp, c_vp],
    "ngp_vm_backward": [c_vp, c_u32, c_vp, c_u32, c_u32, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp],
    "ngp_dnerf_encode": [c_vp, c_vp, c_u32, c_u32, c_vp, c_i32, c_u32, c_vp],
    "ngp_dnerf_grid_points_workspace_bytes": [c_u32, c_u32, c_u32],
    "ngp_dnerf_grid_points": [c_vp, c_u32, c_u32, c_u32, c_f32, c_u32, c_u32, c_u32, c_u32, c_u32, c_vp, c_sz,
                              c_vp, c_vp, c_vp, c_vp],
    "ngp_dnerf_grid_ema_pack": [c_vp, c_vp, c_u32, c_u32, c_u32, c_f32, ctypes.c_double, c_vp, c_vp, c_vp],
}
_RESTYPES = {
    "ngp_last_error": ctypes.c_char_p,
    "ngp_fused_inf_flag": c_vp,
    "ngp_grid_encode_backward_fused_timing_offset": c_sz,
    "ngp_grid_encode_backward_fused_counter_bytes": c_sz,
    "ngp_ffmlp_backward_workspace_bytes": c_sz,
    "ngp_march_rays_train_workspace_bytes": c_sz,
    "ngp_march_rays_train_error_offset": c_sz,
    "ngp_fused_state_bytes": c_sz,
    "ngp_render_state_bytes": c_sz,
    "ngp_render_count": c_vp,
    "ngp_grid_encode_backward_fused_workspace_bytes": c_sz,
    "ngp_ffmlp_image_bytes": c_sz,
    "ngp_nerf_dw_stash_bytes": c_sz,
    "ngp_nerf_backward_join_max_rays": c_u32,
    "ngp_density_grid_draw_workspace_bytes": c_sz,
    "ngp_density_grid_sort_workspace_bytes": c_sz,
    "ngp_density_grid_ostat_workspace_bytes": c_sz,
    "ngp_grad_exchange_bins": c_u32,
    "ngp_grad_exchange_words": ctypes.c_uint64,
    "ngp_mesh_workspace_bytes": c_sz,
    "ngp_mesh_clean_workspace_bytes": c_sz,
    "ngp_background_scratch_bytes": c_sz,
    "ngp_jpeg_scan_capacity": c_sz,
    "ngp_jpeg_workspace_elems": c_sz,
    "ngp_vm_grad_values": c_sz,
    "ngp_vm_backward_scratch_bytes": c_sz,
    "ngp_dnerf_grid_points_workspace_bytes": c_sz,
}

DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.float64: 2}
DTYPE_U8 = 3  # NGP_DTYPE_U8: the image source's pixels only
DENSITY_STATS_LEN = 1025  # include/ngp_hip.h NGP_DENSITY_STATS_LEN (doubles of ngp_density_grid_ema_pack's stats)


class AdamJob(ctypes.Structure):
    """ngp_adam_job (include/ngp_hip.h): the optimizer update a march launch
    carries (ngp_march_rays_train_prebuilt_adam)."""
    _fields_ = [("n_tensors", c_i32), ("params", c_vp * 8), ("grads", c_vp * 8), ("exp_avg", c_vp * 8),
                ("exp_avg_sq", c_vp * 8), ("half_params", c_vp * 8), ("sizes", ctypes.c_uint64 * 8),
                ("lr", c_f32), ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("iters", c_i32),
                ("zero_grads", c_i32), ("grad_mult", c_f32), ("clear", c_vp), ("clear_bytes", c_u32),
                ("flags", c_u32)]


ADAM_JOB_TAIL_LATER = 2  # NGP_ADAM_JOB_TAIL_LATER
ADAM_JOB_EMIT_LAUNCH = 4  # NGP_ADAM_JOB_EMIT_LAUNCH


class BatchJob(ctypes.Structure):
    """ngp_batch_job (include/ngp_hip.h): the fused step's next batch, drawn by
    ngp_grid_encode_backward_fused_reduce_batch."""
    _fields_ = [("poses", c_vp), ("n_poses", c_u32), ("intrinsics4", c_vp), ("H", c_u32), ("W", c_u32),
                ("N", c_u32), ("boxes", c_vp), ("nboxes", c_i32), ("aabb6", c_vp), ("min_near", c_f32),
                ("seed", c_u32), ("state", c_vp), ("rays_o", c_vp), ("rays_d", c_vp), ("rgba", c_vp), ("bg", c_vp),
                ("nears", c_vp), ("fars", c_vp), ("noises", c_vp), ("counter", c_vp), ("step_counter", c_vp)]


class ImageSource(ctypes.Structure):
    """ngp_image_source (include/ngp_hip.h): the pixel stack the fused step's
    batch takes its targets from, and the draw's pixel / image indices; with
    a depth stack, each ray's depths[pose][pix] * depth_scale into depth_out;
    with an error map, the draw's pixels come from ngp_error_map_select's
    `selected` cells and each ray's cell goes to `coarse`."""
    _fields_ = [("pixels", c_vp), ("channels", c_u32), ("dtype", c_i32), ("pix", c_vp), ("image_index", c_vp),
                ("depths", c_vp), ("depth_scale", c_f32), ("depth_out", c_vp),
                ("error_map", c_vp), ("error_map_res", c_u32), ("selected", c_vp), ("perm_mult", c_u32),
                ("coarse", c_vp)]


class DepthLossJob(ctypes.Structure):
    """ngp_depth_loss_job (include/ngp_hip.h): the depth term and the loss
    weights of ngp_nerf_composite_loss_depth, and its optional live-row lists."""
    _fields_ = [("gt_depth", c_vp), ("color_weight", c_f32), ("depth_weight", c_f32), ("depth_min", c_f32),
                ("depth_max", c_f32), ("out_depth", c_vp), ("loss_depth_ray", c_vp), ("ray_rows", c_vp),
                ("live_cnt", c_vp), ("live_rows", c_vp), ("live_total", c_vp)]


class DistLossJob(ctypes.Structure):
    """ngp_dist_loss_job (include/ngp_hip.h): the distortion term's weight and
    its optional per-ray output, of ngp_nerf_composite_loss_dist."""
    _fields_ = [("weight", c_f32), ("loss_dist_ray", c_vp)]


class VMSet(ctypes.Structure):
    """ngp_vm_set (include/ngp_hip.h): three planes [H, W, R] and three lines
    [D, R] of TensoRF's vector-matrix decomposition, and their ranks."""
    _fields_ = [("plane", c_vp * 3), ("line", c_vp * 3), ("rank", c_u32 * 3)]


VM_FIXED_BITS = 32  # NGP_VM_FIXED_BITS
DNERF_ENCODE_COLS = 76  # NGP_DNERF_ENCODE_COLS
DNERF_STATS_LEN = 1025  # NGP_DNERF_STATS_LEN

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the .so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libngp_hip.so not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, ctypes.c_int)
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().ngp_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Raw device pointer of a tensor (or NULL for None)."""
    return None if t is None else t.data_ptr()


def stream_of(t):
    """hipStream_t handle of the current torch stream on the tensor's device."""
    return torch.cuda.current_stream(t.device).cuda_stream


def require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")


def require_contiguous(t, name):
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")


def require_dtype(t, name, dtypes, what):
    if t.dtype not in dtypes:
        raise RuntimeError(f"{name} must be a {what} tensor")


FLOATING = (torch.float32, torch.float16, torch.float64)


def check_tensor(t, name, dtypes=FLOATING, what="floating", contiguous=True):
    require_cuda(t, name)
    if contiguous:
        require_contiguous(t, name)
    if dtypes is not None:
        require_dtype(t, name, dtypes, what)
