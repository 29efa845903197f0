"""Cover-ID algorithms (acoss/algorithms), backed by the HIP engine."""
from .ftm2d import FTM2D  # noqa: F401
