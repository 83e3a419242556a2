"""Training losses whose hot path is a HIP kernel: the ensemble's almost-fair kernel CRPS."""
from .kcrps import CRPS

__all__ = ["CRPS"]
