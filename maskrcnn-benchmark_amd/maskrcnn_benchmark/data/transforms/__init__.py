from .build import build_transforms  # noqa: F401
from .transforms import (ColorJitter, Compose, Normalize, RandomHorizontalFlip, RandomVerticalFlip, RawImage, Resize,  # noqa: F401
                         ToRaw, ToTensor, normalisation_table)
