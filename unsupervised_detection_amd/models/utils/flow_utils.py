"""`from .utils.flow_utils import preprocess_flow_batch` (models/adversarial_learner.py:9)."""
from ...functional import preprocess_flow_batch  # noqa: F401
from ...visualize import flow_to_image  # noqa: F401  (flow_utils.py:74-100, on the device: uint8 tensor out)
