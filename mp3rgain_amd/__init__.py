"""mp3rgain_amd -- MI355X (gfx950) ReplayGain 1.0 analysis path behind mp3rgain's `replaygain` API.

What the hot path needs lives here: `csrc/` (HIP kernels + the C ABI declared in
include/mp3rgain_amd.h), the ctypes binding (`_capi`) and the host-side mirror of the
reference's interface (`replaygain`, `album`).  Either side of the path, as thin mirrors of
the reference's modules over the same library: `mp3gain` (src/lib.rs: lossless global_gain changes, APEv2
undo tags), `mp4meta` (src/mp4meta.rs: ReplayGain tags in M4A files) and `cli` (src/main.rs:
`python -m mp3rgain_amd`).
"""
from . import _capi, replaygain  # noqa: F401
from .mp3verify import Mp3VerifyResult  # noqa: F401
from .replaygain import (  # noqa: F401
    REPLAYGAIN_REFERENCE_DB,
    AlbumGainResult,
    Ancestry,
    AncestryView,
    Analyzer,
    AudioFileType,
    ChannelDynamicRange,
    ChannelSpectrum,
    ChannelStats,
    DynamicRange,
    Fingerprint,
    FlacVerifyResult,
    Node,
    PcmStats,
    PcmTrack,
    PeakAmplitudeResult,
    R128AlbumResult,
    R128Dynamics,
    R128Result,
    ReplayGainError,
    ReplayGainResult,
    RipChecksums,
    RipOffsetSignatures,
    SamePair,
    Spectrum,
    Tempo,
    album_dr,
    ancestry_arena,
    ancestry_from_record,
    ancestry_kernel_shape,
    analyze_album,
    analyze_track,
    dr_arena,
    dr_kernel_shape,
    dynamic_range_from_record,
    find_peak_amplitude,
    fingerprint_arena,
    fingerprint_codes,
    fingerprint_edges,
    fingerprint_from_record,
    fingerprint_groups,
    fingerprint_kernel_shape,
    fingerprint_match_codes,
    is_available,
    pcm_stats_arena,
    pcm_stats_kernel_shape,
    r128_layout_weights,
    rip_offsets_arena,
    rip_offsets_kernel_shape,
    spectrum_arena,
    spectrum_kernel_shape,
    spectrum_verdict,
    tempo_arena,
    tempo_bands,
    tempo_from_onsets,
    tempo_from_record,
    tempo_kernel_shape,
)

__version__ = "0.1.0"
