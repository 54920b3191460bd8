"""neuralcodecs_amd -- MI355X-native Encode/RVQ/Decode engine for DAC / SNAC / Encodec.

The compute lives in ``libnc_mi355x.so`` (hand-written HIP for gfx950 behind the C ABI of
``include/nc_mi355x.h``); this package is the thin host-side mirror of the reference's model
classes (NeuralCodecs.Torch/Models/{DAC,SNAC,Encodec}.cs).
"""
from .config import DACConfig, EncodecConfig, SNACConfig  # noqa: F401
from .dac import DAC, dac_halo, dac_ragged_windows  # noqa: F401
from .snac import SNAC, snac_halo, snac_ragged_windows  # noqa: F401
from .encodec import EncodecCausalPool, EncodecCausalSession, encodec_causal_plan  # noqa: F401
from .encodec import EncodedFrame, Encodec, EncodecStreamPool, EncodecStreamSession, encodec_ragged_rows, encodec_stream_plan  # noqa: F401
from .session import FLUSH, Session, SessionPool, session_pool_plan, session_schedule  # noqa: F401
from .dia import (DiaGeneration, adjust_speed, dia_apply_delay, dia_prefill_pack, dia_revert_delay, dia_sample_host,  # noqa: F401
                  dia_sample_next_token, mix_to_mono_ragged)
from .loudness import LoudnessConfig, apply_gain_db, kweight, normalize_loudness  # noqa: F401
from .loudness import loudness as integrated_loudness  # noqa: F401  (the plain name stays the submodule neuralcodecs_amd.loudness)
from .resample import ResampleConfig, resample_sinc, resample_sinc_geom, resample_sinc_len, resample_sinc_packed, resample_sinc_table  # noqa: F401
from .quality import QualityConfig, mel_filterbank, mel_spectrogram, quality_metrics, stft  # noqa: F401
from .spectral import (dct_matrix, idft_basis, istft, istft_len, istft_packed, mask_frequencies, mask_timesteps, mfcc,  # noqa: F401
                       spectral_mask)

__all__ = ["DAC", "SNAC", "Encodec", "EncodedFrame", "DACConfig", "SNACConfig", "EncodecConfig", "dac_halo", "snac_halo", "dac_ragged_windows",
           "snac_ragged_windows", "encodec_ragged_rows", "encodec_stream_plan", "encodec_causal_plan", "EncodecCausalPool", "EncodecCausalSession", "EncodecStreamPool", "EncodecStreamSession", "Session", "session_schedule", "SessionPool", "FLUSH", "session_pool_plan",
           "adjust_speed", "dia_apply_delay", "dia_revert_delay", "dia_prefill_pack", "mix_to_mono_ragged", "dia_sample_next_token", "dia_sample_host",
           "DiaGeneration", "QualityConfig", "stft", "mel_spectrogram", "mel_filterbank", "quality_metrics",
           "LoudnessConfig", "kweight", "integrated_loudness", "normalize_loudness", "apply_gain_db",
           "ResampleConfig", "resample_sinc", "resample_sinc_packed", "resample_sinc_len", "resample_sinc_geom", "resample_sinc_table",
           "istft", "istft_packed", "istft_len", "mask_frequencies", "mask_timesteps", "mfcc", "dct_matrix", "idft_basis", "spectral_mask"]
from . import audio  # noqa: F401,E402
