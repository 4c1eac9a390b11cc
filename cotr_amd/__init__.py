"""cotr_amd - COTR's batched correspondence-query forward path as hand-written gfx950 (MI355X) HIP
kernels behind a C ABI (``include/cotr_hip.h``), presented through the reference's own Python seam
(``cotr_amd.models.build_model`` == ``COTR.models.build_model``)."""
import argparse

__version__ = '0.1.0'


def default_args(**over):
    """COTR's model defaults (COTR/options/options.py:41-51; dim_feedforward derived from --layer as in
    demo_single_pair.py:58-62)."""
    a = argparse.Namespace(backbone='resnet50', hidden_dim=256, dilation=False, dropout=0.1, nheads=8,
                           layer='layer3', enc_layers=6, dec_layers=6, position_embedding='lin_sine',
                           dim_feedforward=1024)
    for k, v in over.items():
        setattr(a, k, v)
    return a


_DATA_NAMES = ('Capture', 'depth_corrs', 'crop_capture', 'make_batch', 'make_zoom_batch', 'draw_rand', 'rotation_matrix', 'rotated_c2w',
               'rotate_captures', 'rotate_capture', 'rotate_image', 'draw_rotations')
_SCENE_NAMES = ('world_points', 'overlap_pairs', 'overlap_matrix', 'knn_pool', 'draw_pairs')
__all__ = ['default_args'] + list(_DATA_NAMES) + list(_SCENE_NAMES)


def __getattr__(name):
    """the batch builders of cotr_amd/data.py and the pair selection of cotr_amd/scene.py, imported on first use (they bring
    torch and the library binding with them)"""
    if name in _DATA_NAMES:
        from . import data
        return getattr(data, name)
    if name in _SCENE_NAMES:
        from . import scene
        return getattr(scene, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
