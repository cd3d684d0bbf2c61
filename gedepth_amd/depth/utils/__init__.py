from .color_depth import colorize
from .error_bands import ERROR_COLOURS, error_bands
from .point_cloud import POINT_DTYPE, depth_to_points, kitti_intrinsics, scene_records_to_points, write_ply, write_scene_ply
from .position_encoding import SinePositionalEncoding

__all__ = ['SinePositionalEncoding', 'colorize', 'POINT_DTYPE', 'depth_to_points', 'write_ply', 'kitti_intrinsics', 'write_scene_ply',
           'scene_records_to_points']
