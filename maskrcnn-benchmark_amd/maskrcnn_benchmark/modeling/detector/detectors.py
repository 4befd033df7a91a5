"""build_detection_model(cfg) (reference modeling/detector/detectors.py:5-10)."""
from ..make_layers import building
from .generalized_rcnn import GeneralizedRCNN

_DETECTION_META_ARCHITECTURES = {"GeneralizedRCNN": GeneralizedRCNN}


def build_detection_model(cfg):
    with building(cfg):      # GroupNorm layers take MODEL.GROUP_NORM from THIS cfg, not from the global one
        return _DETECTION_META_ARCHITECTURES[cfg.MODEL.META_ARCHITECTURE](cfg)
