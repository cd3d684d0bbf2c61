from .batch_inference import BatchDDADInferencer
from .inference import (inference_depther, inference_error_map, inference_ground, inference_point_cloud, inference_prior_sweep,
                        inference_scene_cloud, init_depther)

__all__ = ['init_depther', 'inference_depther', 'inference_point_cloud', 'inference_ground', 'inference_scene_cloud', 'inference_error_map',
           'inference_prior_sweep', 'BatchDDADInferencer']
