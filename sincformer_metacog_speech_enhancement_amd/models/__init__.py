from .dnn import SpeechEnhancementDNN, create_dnn
from .vq import VectorQuantizer, VQMaskQuantizer
