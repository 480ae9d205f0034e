from .dnn import SpeechEnhancementDNN, create_dnn
from .rbm import RBM, pretrain_dnn_with_rbm, rbm_draws
from .vq import VectorQuantizer, VQMaskQuantizer
