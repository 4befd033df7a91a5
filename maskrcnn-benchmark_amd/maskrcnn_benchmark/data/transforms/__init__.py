from .build import build_transforms, jitter_enabled  # noqa: F401
from .transforms import (ColorJitter, Compose, Normalize, RandomHorizontalFlip, RandomVerticalFlip, RawColorJitter,  # noqa: F401
                         RawImage, Resize, ToRaw, ToTensor, normalisation_table)
