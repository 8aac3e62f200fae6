"""
lhotse_amd -- MI355X-native batched audio feature extraction behind lhotse's
FeatureExtractor interface (see DESIGN.md / INTEGRATION.md).

Importing the package never touches the GPU; extractors create their device plan lazily.
"""
from .extractors import (  # noqa: F401
    HipFbank,
    HipFbankConfig,
    HipLogSpectrogram,
    HipLogSpectrogramConfig,
    HipMfcc,
    HipMfccConfig,
    HipSpectrogram,
    HipSpectrogramConfig,
)

from .augmentation import HipReverb, HipReverbWithImpulseResponse, reverb_in_arena, reverb_tail_floats  # noqa: F401,E402
from .augmentation import REVERB_AUTO_MIN_TAPS, reverb_fft_tail_floats  # noqa: F401,E402
from .augmentation import HipClipping, HipLevel, HipVolume, get_or_create_level, level_in_arena  # noqa: F401,E402
from .augmentation import COLLATE_TILE, HipCollator, collate_in_arena, get_or_create_collator, left_pad_offsets  # noqa: F401,E402
from .augmentation import COLLATE_MAX_SOURCES, collate_sources_in_arena, collate_sources_layout  # noqa: F401,E402
from .augmentation import resample_in_arena, resample_layout, resampled_tail_floats  # noqa: F401,E402
from .augmentation import HipSincResampler, get_or_create_sinc, sinc_in_arena  # noqa: F401,E402
from .augmentation import HipMixer, HipResample, HipResampleTensor, HipSpeed, HipSpeedBank, get_or_create_resampler, mix_in_arena, mixed_tail_floats  # noqa: F401,E402

from .kaldifeat import (  # noqa: F401,E402
    HipKaldifeatFbank,
    HipKaldifeatFbankConfig,
    HipKaldifeatFrameOptions,
    HipKaldifeatMelOptions,
    HipKaldifeatMfcc,
    HipKaldifeatMfccConfig,
)

from .input_strategies import FusedAudioBatch, FusedFeatureBatch, HipAudioSamples, HipOnTheFlyFeatures, HipPrecomputedFeatures  # noqa: F401,E402
from .augmentation import FeatCut, FeatTrack, HipFeatureMixer, featmix_in_arena, featmix_layout, get_or_create_featmixer  # noqa: F401,E402

from .whisper import HipWhisperFbank, HipWhisperFbankConfig  # noqa: F401,E402

from .librosa_fbank import HipLibrosaFbank, HipLibrosaFbankConfig  # noqa: F401,E402

from .signal_transforms import HipGlobalMVN, HipSpecAugment  # noqa: F401,E402

from .stats import GlobalStatsPass, HipStatsAccumulator, compute_global_feature_stats, get_or_create_stats  # noqa: F401,E402

from .layers import HipWav2FFT, HipWav2LogFilterBank, HipWav2LogSpec, HipWav2MFCC, HipWav2Spec, HipWav2Win  # noqa: F401,E402

from .storage import HipArchiveF16Writer, HipArchiveReader, HipArchiveWriter, compute_and_store_features_batch  # noqa: F401,E402

from .sharding import compute_and_store_features_sharded  # noqa: F401,E402

__all__ = [
    "compute_and_store_features_sharded",
    "compute_and_store_features_batch",
    "HipArchiveWriter",
    "HipArchiveF16Writer",
    "HipArchiveReader",
    "HipWhisperFbank",
    "HipLibrosaFbank",
    "HipGlobalMVN",
    "HipStatsAccumulator",
    "GlobalStatsPass",
    "compute_global_feature_stats",
    "get_or_create_stats",
    "HipWav2Win",
    "HipWav2FFT",
    "HipWav2Spec",
    "HipWav2LogSpec",
    "HipWav2LogFilterBank",
    "HipWav2MFCC",
    "HipSpecAugment",
    "HipLibrosaFbankConfig",
    "HipWhisperFbankConfig",
    "HipOnTheFlyFeatures",
    "HipKaldifeatFbank",
    "HipKaldifeatFbankConfig",
    "HipKaldifeatMfcc",
    "HipKaldifeatMfccConfig",
    "HipKaldifeatFrameOptions",
    "HipKaldifeatMelOptions",
    "HipSpeed",
    "HipSpeedBank",
    "HipMixer",
    "mix_in_arena",
    "mixed_tail_floats",
    "HipReverb",
    "HipReverbWithImpulseResponse",
    "reverb_in_arena",
    "reverb_tail_floats",
    "reverb_fft_tail_floats",
    "REVERB_AUTO_MIN_TAPS",
    "HipLevel",
    "HipVolume",
    "HipClipping",
    "get_or_create_level",
    "level_in_arena",
    "COLLATE_TILE",
    "HipCollator",
    "collate_in_arena",
    "COLLATE_MAX_SOURCES",
    "collate_sources_in_arena",
    "collate_sources_layout",
    "get_or_create_collator",
    "left_pad_offsets",
    "FusedAudioBatch",
    "HipAudioSamples",
    "FusedFeatureBatch",
    "HipPrecomputedFeatures",
    "HipFeatureMixer",
    "FeatCut",
    "FeatTrack",
    "featmix_in_arena",
    "featmix_layout",
    "get_or_create_featmixer",
    "resample_in_arena",
    "HipSincResampler",
    "get_or_create_sinc",
    "sinc_in_arena",
    "resample_layout",
    "resampled_tail_floats",
    "HipResample",
    "HipResampleTensor",
    "get_or_create_resampler",
    "HipFbank",
    "HipFbankConfig",
    "HipMfcc",
    "HipMfccConfig",
    "HipSpectrogram",
    "HipSpectrogramConfig",
    "HipLogSpectrogram",
    "HipLogSpectrogramConfig",
]
__version__ = "0.1.0"
