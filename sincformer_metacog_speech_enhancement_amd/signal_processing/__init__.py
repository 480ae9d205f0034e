from .gammatone import GammatoneFilterbank, erb_bandwidth, erb_space, gammatone_impulse_response

__all__ = ["GammatoneFilterbank", "erb_bandwidth", "erb_space", "gammatone_impulse_response"]
