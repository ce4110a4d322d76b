"""ctypes binding of the C-ABI library (include/shw.h).  The HIP library is the product: if it is
missing or cannot be loaded this module raises -- there is no CPU or PyTorch fallback."""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch  # noqa: F401  (imported first on purpose: the process must hold ONE HIP runtime -- torch's)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHW_LIB_PATH") or os.path.join(_HERE, "libshw_hip.so")   # override: kernel A/B builds
CSRC = os.path.join(_HERE, "csrc")

_c_f32p = ctypes.c_void_p     # device pointers of either precision travel as void*
ABI_VERSION = 3           # include/shw.h SHW_ABI_VERSION
CIRCLE_AS_SLICED, CIRCLE_BISECTION, CIRCLE_LEVEL_MEDIAN = 0, 1, 2      # include/shw.h SHW_CIRCLE_*
_SIGNATURES = {
    # name: (restype, argtypes)
    "shw_abi_version": (ctypes.c_int, []),
    "shw_max_points": (ctypes.c_int, []),
    "shw_stiefel_frames": (ctypes.c_int, [_c_f32p, ctypes.c_long, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "shw_ssw_reduce": (ctypes.c_int, [_c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_float, _c_f32p, _c_f32p,
                                      ctypes.c_void_p]),
    "shw_ssw_coef_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_ssw_forward_grad": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p, ctypes.c_void_p,
                                            _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_forward_general": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                               ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_backward_points": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                               ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                               ctypes.c_void_p]),
    "shw_circle_ot": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p,
                                     _c_f32p, ctypes.c_void_p]),
    # gradients w.r.t. the weights on the circle (csrc/shw_ssw_weights.hip): potential rows at the cut the solve left
    "shw_ssw_weight_potentials": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                                 ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_circle_weight_potentials": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                    _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    # float64 path (csrc/shw_ssw_f64.hip): equal sizes, uniform weights
    "shw_max_points_f64": (ctypes.c_int, []),
    "shw_stiefel_frames_f64": (ctypes.c_int, [_c_f32p, ctypes.c_long, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_forward_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_long, ctypes.c_double, _c_f32p, ctypes.c_void_p,
                                           _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_backward_points_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                                   ctypes.c_double, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                   ctypes.c_void_p]),
    "shw_ssw_reduce_f64": (ctypes.c_int, [_c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_f32p, _c_f32p,
                                          ctypes.c_void_p]),
    "shw_circle_ot_f64": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                         ctypes.c_int, _c_f32p, ctypes.c_void_p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    # general float64 path (csrc/shw_ssw_f64_general.hip): weighted and / or unequal-size clouds
    "shw_max_points_f64_general": (ctypes.c_int, []),
    "shw_ssw_forward_general_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long,
                                                   ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_long, ctypes.c_double, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                   ctypes.c_void_p]),
    "shw_ssw_backward_points_general_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int,
                                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                                           ctypes.c_double, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                           ctypes.c_void_p]),
    "shw_circle_ot_general_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                 _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    # points of dimension 2..64 (csrc/shw_ssw_dim.hip): coordinates, circle-level solve, point gradients
    "shw_max_point_dim": (ctypes.c_int, []),
    "shw_stiefel_frames_dim": (ctypes.c_int, [_c_f32p, ctypes.c_long, ctypes.c_int, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_coords_dim": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_long, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_dim_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_ssw_forward_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_long, ctypes.c_float, ctypes.c_void_p, _c_f32p, ctypes.c_void_p,
                                           _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_backward_points_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                                   ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                   ctypes.c_void_p]),
    # gradients with respect to the slicing frames (csrc/shw_ssw_dirs.hip): the coefficient rows folded with d coord / d U
    "shw_ssw_backward_dirs": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p, _c_f32p,
                                             _c_f32p, ctypes.c_void_p]),
    "shw_ssw_backward_dirs_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float,
                                                 _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_ssw_backward_dirs_f64": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_double, _c_f32p,
                                                 _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_esw_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                       ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_esw_backward_points": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_long, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_esw_backward_dirs": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, _c_f32p, ctypes.c_void_p]),
    "shw_esw_forward_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p, _c_f32p, _c_f32p,
                                           ctypes.c_void_p]),
    "shw_esw_backward_points_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_long, _c_f32p, _c_f32p,
                                                   ctypes.c_void_p]),
    "shw_esw_backward_dirs_dim": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_f32p, ctypes.c_void_p]),
    # generalised sliced-W (csrc/shw_gsw.hip): rows of caller-computed keys, and the fused circular defining function
    "shw_gsw_rows_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_float, _c_f32p,
                                            _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_gsw_circular_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_float, _c_f32p,
                                                _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_gsw_circular_backward_points": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_long, ctypes.c_float, _c_f32p, _c_f32p,
                                                        ctypes.c_void_p]),
    "shw_gsw_circular_backward_dirs": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_long, ctypes.c_float, _c_f32p, ctypes.c_void_p]),
    # 1-D optimal transport on the line (csrc/shw_line_ot.hip): unequal sizes and weights, rows of keys or fused projection
    "shw_line_rows_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                             _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, _c_f32p, _c_f32p, _c_f32p,
                                             ctypes.c_void_p]),
    "shw_line_esw_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p, _c_f32p,
                                            ctypes.c_long, ctypes.c_long, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_line_esw_backward_points": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, _c_f32p,
                                                    _c_f32p, ctypes.c_void_p]),
    "shw_line_esw_backward_dirs": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_f32p, ctypes.c_void_p]),
    # ... with the potentials, the gradients w.r.t. the weights: the forward entries' lists plus pot_u, pot_v; the reduction
    "shw_line_rows_forward_pot": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, _c_f32p,
                                                 _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_line_esw_forward_pot": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float, _c_f32p,
                                                _c_f32p, ctypes.c_long, ctypes.c_long, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                                _c_f32p, ctypes.c_void_p]),
    "shw_line_weight_grads_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_line_weight_grads": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, _c_f32p, ctypes.c_void_p]),
    "shw_sinkhorn_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_sinkhorn_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                            _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_sinkhorn_train_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_sinkhorn_forward_train": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                                  _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_sinkhorn_backward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _c_f32p, _c_f32p,
                                             _c_f32p, ctypes.c_void_p]),
    # gradients through the plan and the cost matrix (dense cotangents, each may be null), and the barycentric map
    "shw_sinkhorn_backward_plan": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _c_f32p, _c_f32p,
                                                  _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_sinkhorn_map_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                                _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_sinkhorn_map_backward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _c_f32p, _c_f32p,
                                                 _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_chamfer_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_f32p,
                                           ctypes.c_void_p, _c_f32p, ctypes.c_void_p, _c_f32p, ctypes.c_void_p]),
    "shw_chamfer_backward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _c_f32p,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_f32p, _c_f32p,
                                            ctypes.c_void_p]),
    # exact W for equal-size uniform clouds (csrc/shw_emd.hip): fixed-point auction, one workgroup per pair
    "shw_max_points_emd": (ctypes.c_int, []),
    "shw_emd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "shw_emd_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_float, ctypes.c_void_p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "shw_emd_backward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_void_p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p]),
    # exact W for uniform clouds of different sizes (csrc/shw_emd_units.hip): the same auction on lcm(n, m) units of mass
    "shw_emd_units_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "shw_emd_units_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_emd_units_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_float, ctypes.c_void_p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "shw_emd_units_backward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_void_p, _c_f32p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_float, _c_f32p, _c_f32p,
                                              ctypes.c_void_p]),
    # the sphere map phi (csrc/shw_flow.hip): residual flows on 3-D points from packed effective parameters
    "shw_flow_residual_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_flow_residual_param_count": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "shw_flow_residual_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_flow_residual_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, _c_f32p, ctypes.c_void_p]),
    "shw_flow_residual_backward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p]),
    # the registration network's trunk (csrc/shw_pointnet.hip): PointNet point MLP fused with the max-pool
    "shw_pointnet_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "shw_pointnet_param_count": (ctypes.c_size_t, [ctypes.c_int]),
    "shw_pointnet_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int]),
    "shw_pointnet_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_int, _c_f32p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "shw_pointnet_backward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p, _c_f32p, ctypes.c_long,
                                             ctypes.c_long, ctypes.c_int, _c_f32p, _c_f32p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    # the sphere encoder of the phi-max wrappers (csrc/shw_sphere_map.hip): 3 -> 16 -> 4 -> 2 tanh network, angle map
    "shw_sphere_map_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_sphere_map_param_count": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "shw_sphere_map_backward_blocks": (ctypes.c_int, [ctypes.c_long]),
    "shw_sphere_map_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long]),
    "shw_sphere_map_forward": (ctypes.c_int, [_c_f32p, _c_f32p, ctypes.c_long, _c_f32p, ctypes.c_void_p]),
    "shw_sphere_map_backward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_long, _c_f32p, _c_f32p, _c_f32p,
                                               ctypes.c_void_p]),
    # the registration network after its trunk (csrc/shw_pose.hip): the pose head's six linear layers, the pose update
    "shw_pose_head_supported": (ctypes.c_int, [ctypes.c_int] * 6),
    "shw_pose_head_param_count": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "shw_pose_head_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long] + [ctypes.c_int] * 7),
    "shw_pose_head_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_long] + [ctypes.c_int] * 6
                              + [_c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p]),
    "shw_pose_head_backward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long]
                               + [ctypes.c_int] * 6 + [_c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p]),
    "shw_pose_update_backward_blocks": (ctypes.c_int, [ctypes.c_long]),
    "shw_pose_update_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long]),
    "shw_pose_update_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, _c_f32p,
                                               _c_f32p, _c_f32p, ctypes.c_void_p]),
    "shw_pose_update_backward": (ctypes.c_int, [_c_f32p] * 7 + [ctypes.c_long, ctypes.c_long] + [_c_f32p] * 4
                                 + [ctypes.c_void_p, ctypes.c_void_p]),
    # the sphere encoder of the minibatch Residual-MSSW loss (csrc/shw_mssw.hip): ReLU encoder, i-ResNet flows with a
    # per-point-index scale and shift, angle map
    "shw_mssw_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "shw_mssw_param_count": (ctypes.c_size_t, [ctypes.c_int]),
    "shw_mssw_backward_blocks": (ctypes.c_int, [ctypes.c_long]),
    "shw_mssw_workspace_bytes": (ctypes.c_size_t, [ctypes.c_long, ctypes.c_long, ctypes.c_int]),
    "shw_mssw_forward": (ctypes.c_int, [_c_f32p, _c_f32p, _c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_int, _c_f32p,
                                        ctypes.c_void_p]),
    "shw_mssw_backward": (ctypes.c_int, [_c_f32p] * 4 + [ctypes.c_long, ctypes.c_long, ctypes.c_int] + [_c_f32p] * 3
                          + [ctypes.c_void_p, ctypes.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libshw_hip.so (in-tree) with hipcc; returns the path."""
    cmd = ["make", "-j8", "-C", CSRC] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libshw_hip.so failed:\n" + res.stdout)
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load the HIP library.  Raises if it is absent: the HIP path is the only path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
            "There is no fallback implementation.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)         # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.shw_abi_version() != ABI_VERSION:
        raise RuntimeError("libshw_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError_t {rc}"
                           + (" (invalid value / unsupported size)" if rc == 1 else ""))


def hip_runtimes_mapped() -> list[str]:
    """Paths of every libamdhip64 mapped into this process (should be exactly one)."""
    seen = []
    with open("/proc/self/maps") as fh:
        for line in fh:
            if "libamdhip64" in line:
                path = line.split()[-1]
                if path not in seen:
                    seen.append(path)
    return seen
