from .coco import COCODataset  # noqa: F401
from .cityscapes import CityScapesDataset  # noqa: F401
