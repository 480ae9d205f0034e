from .gammatone import GammatoneFilterbank, erb_bandwidth, erb_space, gammatone_impulse_response
from .features import (FeatureExtractor, bark_to_hz, extract_ams, extract_gfcc, extract_mfcc, extract_rasta_plp, hz_to_bark,
                       hz_to_mel, mel_filterbank, mel_to_hz)
from .haircell import MeddisHairCell

__all__ = ["FeatureExtractor", "GammatoneFilterbank", "MeddisHairCell", "bark_to_hz", "erb_bandwidth", "erb_space", "extract_ams",
           "extract_gfcc", "extract_mfcc", "extract_rasta_plp", "gammatone_impulse_response", "hz_to_bark", "hz_to_mel",
           "mel_filterbank", "mel_to_hz"]
