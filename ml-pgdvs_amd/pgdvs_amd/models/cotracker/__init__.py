"""CoTracker point tracker (pgdvs/models/cotracker/), its correlation step fused in HIP (csrc/cotracker.hip)."""
from .interface import CoTrackerInterface
from .model import CoTracker, build_cotracker
from .predictor import CoTrackerPredictor

__all__ = ["CoTracker", "CoTrackerInterface", "CoTrackerPredictor", "build_cotracker"]
