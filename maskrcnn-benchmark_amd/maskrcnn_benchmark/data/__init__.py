from .synthetic import SyntheticCOCODataset, BatchCollator  # noqa: F401
from .build import make_data_loader  # noqa: F401
