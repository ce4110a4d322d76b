"""MI355X-native spherical sliced-Wasserstein registration loss (+ Chamfer baseline).

Importable as `importlib.import_module("sphere-homeomorphic-wasserstein-distance-for-point-cloud-registration_amd")`
or through the top-level alias module `shw_amd`."""
from . import _lib, dist
from .chamfer import chamfer_distance, chamfer_pair_losses
from .emd import (Cos_disimilarity_W, Geodesic_distance_W, emd_pair_costs, max_points_emd, transport_pair_costs,
                  transport_units, wasserstein_distance, wasserstein_distance_geo)
from .esw import (augmented_sliced_wassersten_distance, augmented_sliced_wasserstein_distance, esw_slice_sums,
                  max_sliced_wasserstein_distance, rand_projections, sliced_wasserstein_distance)
from .flows import (Norm_Flow_structure, Norm_Flow_structure_optuna, residual_flow, residual_flow_composed,
                    residual_flow_supported, residual_param_count)
from .gsw import (GSWD_circular, GSWD_polynomial, cosine_distance_torch, distributional_sliced_wasserstein_distance,
                  gsw_circular_slice_sums, gsw_nn_1, gsw_nn_3, gsw_polynomial_slice_sums, max_GSWD_circular,
                  max_GSWD_polynomial_3, max_GSWD_polynomial_5, max_gsw_nn_1, max_gsw_nn_3, poly_degree, sorted_row_sums)
from . import mssw
from .line_ot import esw_slice_costs, line_ot_rows, weighted_sliced_wasserstein_distance
from .modules import (ChamferCriterion, GraphedAscent, GraphedStep, SlicedSphereW, SSWCriterion, max_cos_disimilarity_wassersten_distance,
                      max_spherical_wassersten_distance, max_spherical_wassersten_distance_fast)
from .mssw import (ActNorm, Flow_structure, max_spherical_wassersten_distance_Residual, residual_sphere_map,
                   residual_sphere_map_composed)
from .mssw import transform_to_sphere as transform_to_sphere_Residual
from .pcrnet import (MLP_Architecture, PCRNet, Pooling, convert2transformation, create_pose_7d, get_quaternion,
                     get_translation, pointnet_max_features, pointnet_max_features_composed, pointnet_param_count,
                     pointnet_supported, qrot, quaternion_rotate, quaternion_transform, unpack_pointnet_params)
from .pose import (pose_head, pose_head_composed, pose_head_param_count, pose_head_supported, pose_update,
                   pose_update_composed, unpack_pose_head_params)
from .sinkhorn import (log_N_Sinkhorn_Distance_Loss, log_Sinkhorn_Distance_Loss, sinkhorn_barycentric_map,
                       sinkhorn_pair_costs)
from .sphere_map import sphere_map, sphere_map_composed, transform_to_sphere, transform_to_sphere_fast
from .ssw import (binary_search_circle, circle_coordinates, draw_directions, emd1D_circle, enable_float64, enable_float64_general, float64_enabled,
                  float64_general_enabled, max_points_f64, max_points_f64_general, max_sliced_wasserstein_sphere, retract_frames, stiefel_frames, sliced_cost, sliced_wasserstein_sphere, sliced_wasserstein_sphere_fast,
                  ssw_pair_losses)

__all__ = ["_lib", "dist", "binary_search_circle", "circle_coordinates", "emd1D_circle", "enable_float64", "enable_float64_general", "float64_enabled", "float64_general_enabled", "max_points_f64",
           "max_points_f64_general", "ChamferCriterion", "GraphedAscent", "GraphedStep", "SlicedSphereW", "SSWCriterion",
           "max_spherical_wassersten_distance", "max_spherical_wassersten_distance_fast",
           "max_cos_disimilarity_wassersten_distance", "chamfer_distance", "chamfer_pair_losses", "draw_directions", "log_N_Sinkhorn_Distance_Loss", "log_Sinkhorn_Distance_Loss", "sinkhorn_barycentric_map", "sinkhorn_pair_costs", "stiefel_frames", "augmented_sliced_wassersten_distance", "augmented_sliced_wasserstein_distance", "esw_slice_sums", "rand_projections", "sliced_wasserstein_distance", "sliced_cost", "sliced_wasserstein_sphere", "sliced_wasserstein_sphere_fast",
           "ssw_pair_losses", "max_sliced_wasserstein_sphere", "retract_frames", "GSWD_circular", "GSWD_polynomial", "cosine_distance_torch",
           "distributional_sliced_wasserstein_distance", "gsw_circular_slice_sums", "gsw_nn_1", "gsw_nn_3",
           "gsw_polynomial_slice_sums", "max_GSWD_circular", "max_GSWD_polynomial_3", "max_GSWD_polynomial_5",
           "max_gsw_nn_1", "max_gsw_nn_3", "poly_degree", "sorted_row_sums", "esw_slice_costs", "line_ot_rows",
           "weighted_sliced_wasserstein_distance", "Cos_disimilarity_W", "Geodesic_distance_W", "emd_pair_costs",
           "max_points_emd", "wasserstein_distance", "wasserstein_distance_geo", "transport_pair_costs",
           "transport_units", "Norm_Flow_structure", "Norm_Flow_structure_optuna", "residual_flow",
           "residual_flow_composed", "residual_flow_supported", "residual_param_count", "MLP_Architecture", "PCRNet",
           "Pooling", "convert2transformation", "create_pose_7d", "get_quaternion", "get_translation",
           "pointnet_max_features", "pointnet_max_features_composed", "pointnet_param_count", "pointnet_supported", "qrot",
           "quaternion_rotate", "quaternion_transform", "unpack_pointnet_params", "sphere_map", "sphere_map_composed",
           "transform_to_sphere", "transform_to_sphere_fast", "pose_head", "pose_head_composed", "pose_head_param_count",
           "pose_head_supported", "pose_update", "pose_update_composed", "unpack_pose_head_params", "mssw",
           "max_spherical_wassersten_distance_Residual", "Flow_structure", "ActNorm", "transform_to_sphere_Residual",
           "residual_sphere_map", "residual_sphere_map_composed"]
