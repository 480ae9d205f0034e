"""Constants of the reference's config.py that the hot path reads
(config.py:17-21 audio framing, :93-98 Conformer, :105-107 agents, :25 channels).
Only values are mirrored; nothing else of the reference configuration exists here."""
import os as _os

# checkpoints (config.py:13 of the reference: <repo>/saved_models); override with SFM_MODEL_DIR
MODEL_DIR = _os.environ.get("SFM_MODEL_DIR") or _os.path.join(_os.getcwd(), "saved_models")

SAMPLE_RATE = 8000
FRAME_SIZE_MS = 20
FRAME_SIZE = int(SAMPLE_RATE * FRAME_SIZE_MS / 1000)   # 160
HOP_SIZE = FRAME_SIZE // 2                              # 80
FFT_SIZE = 256
NUM_CHANNELS = 64
# the gammatone filterbank (config.py:26-28 of the reference)
FREQ_LOW = 50
FREQ_HIGH = 4000
FILTER_ORDER = 4
# the DNN front end (config.py:31-46 of the reference): AMS, MFCC, GFCC, RASTA-PLP and the context
AMS_SEGMENTS = 128
AMS_OVERLAP = 64
AMS_FFT_SIZE = 256
AMS_NUM_BANDS = 15
MFCC_NUM_COEFF = 13
MFCC_FFT_SIZE = 512
MFCC_NUM_FILTERS = 64
GFCC_NUM_COEFF = 13
GFCC_DECIMATE_RATE = 100
RASTA_NUM_COEFF = 13
CONTEXT_FRAMES = 5
# the mask-estimating DNN (config.py:64-72 of the reference)
DNN_HIDDEN_LAYERS = 3
DNN_HIDDEN_UNITS = 1024
DNN_DROPOUT = 0.2
DNN_LEARNING_RATE = 0.001
DNN_EPOCHS = 50
DNN_BATCH_SIZE = 256
# the RBM pre-training of the DNN (config.py:75-78 of the reference)
RBM_LEARNING_RATE = 0.01
RBM_EPOCHS = 10
RBM_BATCH_SIZE = 256
RBM_K_STEPS = 1
CONFORMER_NUM_BLOCKS = 6
CONFORMER_D_MODEL = 256
CONFORMER_NUM_HEADS = 4
CONFORMER_FF_DIM = 1024
CONFORMER_KERNEL_SIZE = 31
CONFORMER_DROPOUT = 0.1
CPEA_HIDDEN_SIZE = 128
CPEA_NUM_LAYERS = 2
PA_ENCODER_CHANNELS = 256

# SURVEY 8f N4 (config.py:101-108 of the reference)
VQ_NUM_CENTROIDS = 3
VQ_COMMITMENT_WEIGHT = 0.25
MAA_THRESHOLD_INIT = 0.5

# OPT-PCIRM quantiser (config.py:89-90 of the reference): M = 3 attenuation steps, local criterion -15 dB
OPT_NUM_STEPS = 3
LOCAL_CRITERION_DB = -15

# the swarm that searches OPT-PCIRM's middle step (config.py:81-86 of the reference)
PSO_NUM_PARTICLES = 30
PSO_MAX_ITER = 100
PSO_W = 0.7
PSO_C1 = 1.5
PSO_C2 = 1.5
PSO_BOUNDS = (0.0, 1.0)

# evaluation/stoi.py of the reference asks pystoi for the extended measure (config.py:116 of the reference)
STOI_EXTENDED = False

# curriculum stages in epochs (config.py:120-122 of the reference)
CURRICULUM_STAGE1_EPOCHS = 15
CURRICULUM_STAGE2_EPOCHS = 20
CURRICULUM_STAGE3_EPOCHS = 15
