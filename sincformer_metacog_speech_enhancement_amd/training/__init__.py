from .curriculum import CurriculumScheduler
from .losses import MSEMaskLoss, PerceptualSTOILoss

__all__ = ["CurriculumScheduler", "MSEMaskLoss", "PerceptualSTOILoss"]
