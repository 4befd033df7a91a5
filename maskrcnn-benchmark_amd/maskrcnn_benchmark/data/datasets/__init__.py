from .coco import COCODataset  # noqa: F401
