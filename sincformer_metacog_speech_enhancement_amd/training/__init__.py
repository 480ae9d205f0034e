from .conformer_pipeline import (CurriculumBatch, NoiseBank, WarmupCosineRule, WaveformSet, curriculum_batch, mix_at_snr,
                                 mix_batch)
from .curriculum import CurriculumScheduler
from .pipeline import dnn_enhance_signal, dnn_estimate_mask, dnn_frame_pairs, gammatone_mask_target, rbm_pretrain, resynthesize
from .dnn_training import FrameSet, PlateauRule, TrainingPipeline
from .losses import AdversarialLoss, MSEMaskLoss, PerceptualSTOILoss, SubDiscriminator, TaalSTOILoss

__all__ = ["AdversarialLoss", "CurriculumBatch", "CurriculumScheduler", "FrameSet", "MSEMaskLoss", "NoiseBank", "PerceptualSTOILoss",
           "PlateauRule", "SubDiscriminator", "TaalSTOILoss", "TrainingPipeline", "WarmupCosineRule", "WaveformSet", "curriculum_batch",
           "dnn_enhance_signal", "dnn_estimate_mask", "dnn_frame_pairs", "gammatone_mask_target", "mix_at_snr", "mix_batch",
           "rbm_pretrain", "resynthesize"]
