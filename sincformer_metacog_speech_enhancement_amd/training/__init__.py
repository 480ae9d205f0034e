from .curriculum import CurriculumScheduler
from .losses import AdversarialLoss, MSEMaskLoss, PerceptualSTOILoss, SubDiscriminator

__all__ = ["AdversarialLoss", "CurriculumScheduler", "MSEMaskLoss", "PerceptualSTOILoss", "SubDiscriminator"]
