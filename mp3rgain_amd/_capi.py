"""ctypes binding of include/mp3rgain_amd.h (the C-ABI drop-in boundary).

This module only loads the in-tree shared library and declares signatures; there is no
Python or CPU compute path behind it.  If the library is missing it raises, loudly.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
import os

# MP3RGAIN_AMD_LIB selects another build of the same library (kernel experiments); never a fallback
LIB_PATH = Path(os.environ.get("MP3RGAIN_AMD_LIB", PKG_DIR / "libmp3rgain_amd.so"))

HISTOGRAM_SIZE = 12000
COMM_ID_BYTES = 128
HISTOGRAM_OFFSET = 2000
FMT_F32_PLANAR, FMT_S16_PLANAR, FMT_S32_PLANAR = 0, 1, 2

RG_OK = 0
RG_ERR_INVALID_ARG = -1
RG_ERR_UNSUPPORTED_RATE = -2
RG_ERR_DEVICE = -3
RG_ERR_NO_DEVICE = -4
RG_ERR_NOMEM = -5
RG_ERR_STATE = -6
RG_ERR_COLLECTIVE = -7


class TrackDesc(C.Structure):
    _fields_ = [
        ("offset_bytes", C.c_uint64),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint16),
        ("format", C.c_uint16),
    ]


class TrackResult(C.Structure):
    _fields_ = [
        ("loudness_db", C.c_double),
        ("gain_db", C.c_double),
        ("peak", C.c_double),
        ("sample_rate", C.c_uint32),
        ("gain_steps", C.c_int32),
        ("windows", C.c_uint32),
        ("file_type", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AlbumResult(C.Structure):
    _fields_ = [
        ("album_loudness_db", C.c_double),
        ("album_gain_db", C.c_double),
        ("album_peak", C.c_double),
        ("album_gain_steps", C.c_int32),
        ("windows", C.c_uint32),
    ]


class PeakResult(C.Structure):
    _fields_ = [
        ("peak", C.c_double),
        ("peak_pcm", C.c_double),
        ("sample_rate", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class R128TrackResult(C.Structure):  # include/mp3rgain_amd_r128.h
    _fields_ = [
        ("loudness_lufs", C.c_double),
        ("gain_db", C.c_double),
        ("sample_peak", C.c_double),
        ("true_peak", C.c_double),
        ("sample_rate", C.c_uint32),
        ("blocks", C.c_uint32),
        ("blocks_gated", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class R128AlbumResult(C.Structure):
    _fields_ = [
        ("loudness_lufs", C.c_double),
        ("gain_db", C.c_double),
        ("sample_peak", C.c_double),
        ("true_peak", C.c_double),
        ("blocks", C.c_uint32),
        ("blocks_gated", C.c_uint32),
    ]


class R128ChannelWeights(C.Structure):  # rg_r128_channel_weights
    _fields_ = [("w", C.c_double * 8)]


R128_CHANNELS_PAIR, R128_CHANNELS_LAYOUT = 0, 1


class R128Dynamics(C.Structure):  # rg_r128_dynamics
    _fields_ = [
        ("loudness_range_lu", C.c_double),
        ("range_low_lufs", C.c_double),
        ("range_high_lufs", C.c_double),
        ("max_momentary_lufs", C.c_double),
        ("max_short_term_lufs", C.c_double),
        ("st_blocks", C.c_uint32),
        ("st_blocks_gated", C.c_uint32),
    ]


class DeviceView(C.Structure):
    _fields_ = [
        ("d_track_hist", C.c_void_p),
        ("d_track_result", C.c_void_p),
        ("d_album_hist", C.c_void_p),
        ("d_album_peak", C.c_void_p),
        ("n_tracks", C.c_uint64),
    ]


# every symbol include/mp3rgain_amd.h declares: (name, restype, argtypes)
_vp, _sz, _u32, _i32, _u64, _dbl, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_uint64, C.c_double, C.c_int
_P = C.POINTER
class WavInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint16), ("bits_per_sample", C.c_uint16),
                ("sample_format", C.c_uint16), ("block_align", C.c_uint16), ("reserved", C.c_uint32),
                ("data_offset", C.c_uint64), ("frames", C.c_uint64)]


SYMBOLS = [
    ("rg_abi_version", _int, []),
    ("rg_is_available", _int, []),
    ("rg_supported_rate", _int, [_u32]),
    ("rg_window_samples", _u32, [_u32]),
    ("rg_hist_loudness", _dbl, [_vp]),
    ("rg_gain_from_loudness", _dbl, [_dbl]),
    ("rg_gain_steps", _i32, [_dbl]),
    ("rg_db_to_steps", _i32, [_dbl]),
    ("rg_steps_to_db", _dbl, [_i32]),
    ("rg_clip_limit_steps", _i32, [_i32, _dbl, _dbl, _int, _int]),
    ("rg_rate_design_info", _int, [_u32, _P(_int), _P(_u32), _P(_dbl)]),
    ("rg_create", _vp, [_int]),
    ("rg_destroy", None, [_vp]),
    ("rg_last_error", C.c_char_p, [_vp]),
    ("rg_set_stream", _int, [_vp, _vp, _int]),
    ("rg_wait_user_stream", _int, [_vp]),
    ("rg_batch_stream", _vp, [_vp]),
    ("rg_set_kernel", _int, [_vp, _int]),
    ("rg_set_tuning", _int, [_vp, _int, C.c_int64]),
    ("rg_tm_design_info", _int, [_u32, _u32, _P(_u32), _P(_u32), _P(_u32), _P(_dbl), _vp, _vp]),
    ("rg_tm_design_affine", _int, [_u32, _u32, _P(_int), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _vp]),
    ("rg_analyze_pcm_batch", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _P(TrackResult), _vp]),
    ("rg_analyze_album_pcm", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _P(TrackResult), _P(AlbumResult), _vp]),
    ("rg_find_peak_pcm", _int, [_vp, _P(TrackDesc), _vp, _sz, _int, _P(PeakResult)]),
    ("rg_enqueue_pcm_batch", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int]),
    ("rg_device_view_get", _int, [_vp, _P(DeviceView)]),
    ("rg_collect", _int, [_vp, _P(TrackResult), _vp]),
    ("rg_collect_exact", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _P(TrackResult), _vp]),
    ("rg_album_allreduce", _int, [_vp, _vp]),
    ("rg_album_finish", _int, [_vp, _P(AlbumResult), _vp]),
    ("rg_comm_library", _int, [C.c_char_p]),
    ("rg_comm_unique_id", _int, [_vp]),
    ("rg_comm_init", _int, [_vp, _vp, _int, _int]),
    ("rg_comm_destroy", _int, [_vp]),
    ("rg_comm_info", _int, [_vp, _P(_int), _P(_int)]),
    ("rg_album_exchange", _int, [_vp]),
    ("rg_album_reduce_gathered", _int, [_vp, _vp, _u32]),
    ("rg_album_result_enqueue", _int, [_vp]),
    ("rg_timing_enable", _int, [_vp, _int]),
    ("rg_timing_read", _int, [_vp, _P(_dbl), _P(_u64), _P(_dbl), _int]),
    ("rg_synth_fill_device", _int, [_vp, _vp, _u64, _u32, _u32, _u64, _u64]),
    ("rg_wav_parse", _int, [_vp, _sz, _P(WavInfo)]),
    ("rg_set_decoder_command", _int, [_vp, C.c_char_p]),
    ("rg_analyze_wav_batch", _int, [_vp, _P(_vp), _P(_sz), _sz, _int, _P(TrackResult), _P(AlbumResult)]),
    ("rg_analyze_track", _int, [_vp, C.c_char_p, _i32, _P(TrackResult)]),
    ("rg_analyze_album", _int, [_vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(AlbumResult)]),
    ("rg_analyze_tracks", _int, [_vp, C.POINTER(C.c_char_p), C.c_size_t, C.c_int32, _P(TrackResult), C.POINTER(C.c_int32)]),
    ("rg_tracks_error", C.c_char_p, [_vp, C.c_size_t]),
    ("rg_find_peak_amplitude", _int, [_vp, C.c_char_p, _P(PeakResult)]),
    ("rg_mp3_decode_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("rg_mp3_decode_bench", _int, [_vp, _vp, _sz, _u32, _u32, _P(_dbl), _P(_u64), _P(_u64), _P(_u64)]),
    ("rg_analyze_album_begin", _int, [_vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(_sz)]),
    ("rg_analyze_albums", _int, [_vp, _P(C.c_char_p), _sz, _P(_sz), _sz, _i32, _P(TrackResult), _P(_i32), _P(AlbumResult), _P(_i32)]),
    # include/mp3rgain_amd_node.h
    ("rg_node_create", _vp, [_P(_int), _sz]),
    ("rg_node_create_backend", _vp, [_vp, _P(_int), _sz]),
    ("rg_node_destroy", None, [_vp]),
    ("rg_node_last_error", C.c_char_p, [_vp]),
    ("rg_node_devices", _sz, [_vp]),
    ("rg_node_ctx", _vp, [_vp, _sz]),
    ("rg_node_set_exchange", _int, [_vp, _int]),
    ("rg_node_partition", None, [_P(_u64), _sz, _sz, _P(_u32)]),
    ("rg_analyze_album_node", _int, [_vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(AlbumResult)]),
    ("rg_analyze_tracks_node", _int, [_vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(_i32)]),
    ("rg_node_tracks_error", C.c_char_p, [_vp, _sz]),
    ("rg_node_last_partition", _int, [_vp, _P(_u32), _sz]),
    ("rg_analyze_albums_node", _int, [_vp, _P(C.c_char_p), _sz, _P(_sz), _sz, _i32, _P(TrackResult), _P(_i32), _P(AlbumResult), _P(_i32)]),
]

# include/mp3rgain_amd_r128.h (EBU R 128 / ReplayGain 2.0): a header of its own, bound beside SYMBOLS
R128_SYMBOLS = [
    ("rg_r128_supported_rate", _int, [_u32]),
    ("rg_r128_design_info", _int, [_u32, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_u32), _P(_u32)]),
    ("rg_r128_block_count", _u64, [_u32, _u64]),
    ("rg_r128_set_tuning", _int, [_vp, _int, C.c_int64]),
    ("rg_r128_analyze_pcm_batch", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _int, _P(R128TrackResult), _vp]),
    ("rg_r128_analyze_album_pcm", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _int, _P(R128TrackResult), _P(R128AlbumResult), _vp]),
    ("rg_r128_analyze_tracks", _int, [_vp, _P(C.c_char_p), _sz, _i32, _int, _P(R128TrackResult), _P(_i32)]),
    ("rg_r128_analyze_album", _int, [_vp, _P(C.c_char_p), _sz, _i32, _int, _P(R128TrackResult), _P(R128AlbumResult)]),
    # loudness range and momentary / short-term maxima
    ("rg_r128_short_term_count", _u64, [_u32, _u64]),
    ("rg_r128_analyze_pcm_batch_dynamics", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _int, _P(R128TrackResult), _vp,
                                                  _P(R128Dynamics), _vp]),
    ("rg_r128_analyze_album_pcm_dynamics", _int, [_vp, _P(TrackDesc), _sz, _vp, _sz, _int, _int, _P(R128TrackResult), _P(R128AlbumResult),
                                                  _vp, _P(R128Dynamics), _P(R128Dynamics), _vp]),
    ("rg_r128_analyze_tracks_dynamics", _int, [_vp, _P(C.c_char_p), _sz, _i32, _int, _P(R128TrackResult), _P(_i32), _P(R128Dynamics)]),
    ("rg_r128_analyze_album_dynamics", _int, [_vp, _P(C.c_char_p), _sz, _i32, _int, _P(R128TrackResult), _P(R128AlbumResult),
                                              _P(R128Dynamics), _P(R128Dynamics)]),
    # many albums in one call, and the node
    ("rg_r128_album_select_form", _int, [_int, _u64]),
    ("rg_r128_albums_count_workgroups", _u32, [_u64]),
    ("rg_r128_albums_wide_rounds", _sz, [_sz, _P(_sz)]),
    ("rg_r128_analyze_albums_pcm", _int, [_vp, _P(TrackDesc), _sz, _P(_sz), _sz, _vp, _sz, _int, _int, _P(R128TrackResult),
                                          _P(R128AlbumResult), _vp]),
    ("rg_r128_analyze_albums_pcm_dynamics", _int, [_vp, _P(TrackDesc), _sz, _P(_sz), _sz, _vp, _sz, _int, _int, _P(R128TrackResult),
                                                   _P(R128AlbumResult), _vp, _P(R128Dynamics), _P(R128Dynamics), _vp]),
    ("rg_r128_analyze_albums", _int, [_vp, _P(C.c_char_p), _sz, _P(_sz), _sz, _i32, _int, _P(R128TrackResult), _P(_i32),
                                      _P(R128AlbumResult), _P(_i32)]),
    ("rg_r128_analyze_albums_dynamics", _int, [_vp, _P(C.c_char_p), _sz, _P(_sz), _sz, _i32, _int, _P(R128TrackResult), _P(_i32),
                                               _P(R128AlbumResult), _P(_i32), _P(R128Dynamics), _P(R128Dynamics)]),
    ("rg_r128_layout_weights", _int, [_u32, _u32, _P(R128ChannelWeights)]),
    ("rg_r128_set_channel_mode", _int, [_vp, _int]),
    ("rg_r128_analyze_pcm_weighted", _int, [_vp, _P(TrackDesc), _P(R128ChannelWeights), _sz, _P(_sz), _sz, _vp, _sz, _int, _int,
                                            _P(R128TrackResult), _P(R128AlbumResult), _vp, _P(R128Dynamics), _P(R128Dynamics), _vp]),
    ("rg_r128_analyze_tracks_node", _int, [_vp, _P(C.c_char_p), _sz, _i32, _int, _P(R128TrackResult), _P(_i32), _P(R128Dynamics)]),
    ("rg_r128_analyze_albums_node", _int, [_vp, _P(C.c_char_p), _sz, _P(_sz), _sz, _i32, _int, _P(R128TrackResult), _P(_i32),
                                           _P(R128AlbumResult), _P(_i32), _P(R128Dynamics), _P(R128Dynamics)]),
]

# include/mp3rgain_amd_rip.h (rip checksums: CRC-32 and AccurateRip v1 / v2 per track)
RIP_FIRST_TRACK, RIP_LAST_TRACK = 1, 2
RIP_CD_RATE, RIP_CD_FRAMES, RIP_COMPLETE = 1, 2, 4
RIP_OFFSET_MAX, RIP_DISC_MAX_TRACKS = 2939, 1024


class RipRecord(C.Structure):  # rg_rip_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("null_samples", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("crc32", C.c_uint32),
        ("crc32_nonnull", C.c_uint32),
        ("arv1", C.c_uint32),
        ("arv2", C.c_uint32),
    ]


RIP_SYMBOLS = [
    ("rg_rip_checksums", _int, [_vp, _P(C.c_char_p), _sz, _P(_u32), _P(RipRecord)]),
    ("rg_rip_checksums_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(_u32), _vp, _sz, _P(RipRecord)]),
    ("rg_rip_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32)]),
    ("rg_rip_crc32_algebra", _int, [_u32, _u32, _u64, _P(_u32), _P(_u32)]),
    ("rg_rip_rate", _int, [_vp, _sz, _u64, _int, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_sz)]),
    ("rg_rip_offset_signatures", _int, [_vp, _P(C.c_char_p), _sz, _P(_u32), C.c_int32, _P(RipRecord), _P(_u32), _P(_u32)]),
    ("rg_rip_offsets_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(_u32), C.c_int32, _vp, _sz, _P(_u32), _P(_u32)]),
    ("rg_rip_offsets_kernel_shape", _int, [_P(_u32), _P(_u32)]),
    ("rg_rip_offsets_rate", _int, [_vp, _sz, _u64, C.c_int32, _u32, _u32, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_u64), _P(_u64), _P(_sz)]),
]

# include/mp3rgain_amd_stats.h (PCM defect scan: clipping runs, dropouts, DC, padded bits)
STATS_CLIPPED, STATS_DROPOUT, STATS_PADDED, STATS_NONFINITE, STATS_SILENT, STATS_COMPLETE = 1, 2, 4, 8, 16, 32
STATS_MAX_CHANNELS, STATS_MIN_CLIP_RUN, STATS_MIN_ZERO_RUN = 8, 3, 64


class PcmStatsOpts(C.Structure):  # rg_pcm_stats_opts
    _fields_ = [("min_clip_run", C.c_uint32), ("min_zero_run", C.c_uint32)]


class PcmStatsChannel(C.Structure):  # rg_pcm_stats_channel
    _fields_ = [
        ("min", C.c_double),
        ("max", C.c_double),
        ("sum", C.c_int64),
        ("or_mask", C.c_uint32),
        ("effective_bits", C.c_uint32),
        ("clipped", C.c_uint32),
        ("clip_runs", C.c_uint32),
        ("longest_clip_run", C.c_uint32),
        ("first_clip_run", C.c_uint32),
        ("zeros", C.c_uint32),
        ("lead_zeros", C.c_uint32),
        ("trail_zeros", C.c_uint32),
        ("zero_runs", C.c_uint32),
        ("longest_zero_run", C.c_uint32),
        ("nonfinite", C.c_uint32),
    ]


class PcmStatsRecord(C.Structure):  # rg_pcm_stats_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("bits", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("lead_silence_frames", C.c_uint32),
        ("trail_silence_frames", C.c_uint32),
        ("reserved", C.c_uint32),
        ("ch", PcmStatsChannel * STATS_MAX_CHANNELS),
    ]


STATS_SYMBOLS = [
    ("rg_pcm_stats", _int, [_vp, _P(C.c_char_p), _sz, _P(PcmStatsOpts), _P(PcmStatsRecord)]),
    ("rg_pcm_stats_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(_u32), _P(PcmStatsOpts), _vp, _sz, _P(PcmStatsRecord)]),
    ("rg_pcm_stats_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32)]),
    ("rg_pcm_stats_rate", _int, [_vp, _sz, _u64, _u32, _int, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz)]),
]

# include/mp3rgain_amd_spectrum.h (spectral scan: band spectrum, cutoff, upsampled files)
SPEC_BANDLIMITED, SPEC_UPSAMPLED, SPEC_SHORT, SPEC_NONFINITE, SPEC_COMPLETE = 1, 2, 4, 8, 16
SPEC_MAX_CHANNELS, SPEC_FRAME, SPEC_HOP, SPEC_BANDS = 8, 4096, 2048, 256
SPEC_EDGE_DB, SPEC_MIN_CUTOFF_HZ = 30.0, 4000.0


class SpectrumOpts(C.Structure):  # rg_spectrum_opts
    _fields_ = [("edge_db", C.c_double), ("min_cutoff_hz", C.c_double)]


class SpectrumChannel(C.Structure):  # rg_spectrum_channel
    _fields_ = [
        ("cutoff_hz", C.c_double),
        ("edge_db", C.c_double),
        ("analysed_frames", C.c_uint32),
        ("skipped_frames", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SpectrumRecord(C.Structure):  # rg_spectrum_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("cutoff_hz", C.c_double),
        ("ch", SpectrumChannel * SPEC_MAX_CHANNELS),
    ]


SPECTRUM_SYMBOLS = [
    ("rg_spectrum", _int, [_vp, _P(C.c_char_p), _sz, _P(SpectrumOpts), _P(SpectrumRecord), _P(_dbl)]),
    ("rg_spectrum_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(SpectrumOpts), _vp, _sz, _P(SpectrumRecord), _P(_dbl)]),
    ("rg_spectrum_verdict", _int, [_P(_dbl), _u32, _u32, _P(SpectrumOpts), _P(SpectrumChannel)]),
    ("rg_spectrum_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_spectrum_rate", _int, [_vp, _sz, _u64, _u32, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_sz)]),
]

# include/mp3rgain_amd_dr.h (dynamic range: per-block RMS and peaks, the loudest fifth of the blocks)
DR_COMPLETE, DR_SILENT, DR_NONFINITE, DR_SHORT = 1, 2, 4, 8
DR_MAX_CHANNELS, DR_TOP_PERMILLE, DR_MAX_BLOCK_FRAMES = 8, 200, 1152000


class DrOpts(C.Structure):  # rg_dr_opts
    _fields_ = [("block_frames", C.c_uint32), ("top_permille", C.c_uint32)]


class DrChannel(C.Structure):  # rg_dr_channel
    _fields_ = [
        ("dr", C.c_double),
        ("peak_db", C.c_double),
        ("rms_db", C.c_double),
        ("top_ms", C.c_double),
        ("mean_square", C.c_double),
        ("peak", C.c_uint32),
        ("peak2", C.c_uint32),
        ("blocks", C.c_uint32),
        ("top_blocks", C.c_uint32),
        ("nonfinite", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class DrRecord(C.Structure):  # rg_dr_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("block_frames", C.c_uint32),
        ("dr", C.c_int32),
        ("dr_mean", C.c_double),
        ("peak_db", C.c_double),
        ("rms_db", C.c_double),
        ("ch", DrChannel * DR_MAX_CHANNELS),
    ]


DR_SYMBOLS = [
    ("rg_dynamic_range", _int, [_vp, _P(C.c_char_p), _sz, _P(DrOpts), _P(DrRecord)]),
    ("rg_dr_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(DrOpts), _vp, _sz, _P(DrRecord)]),
    ("rg_dr_kernel_shape", _int, [_u32, _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_dr_rate", _int, [_vp, _sz, _u64, _u32, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz), _P(_u64)]),
]

# include/mp3rgain_amd_stereo.h (stereo image: moments of channels 0 and 1, raw comparisons, cross-correlation at every lag)
(ST_COMPLETE, ST_SILENT, ST_NONFINITE, ST_DUAL_MONO, ST_INVERTED_COPY, ST_OUT_OF_PHASE, ST_NEAR_MONO, ST_ONE_SIDED, ST_DELAYED, ST_MONO,
 ST_MORE_CHANNELS) = (1 << k for k in range(11))
ST_MAX_CHANNELS, ST_MAX_RADIUS, ST_MAX_BLOCK_FRAMES = 8, 255, 384000
ST_DEFAULT_RADIUS, ST_DEFAULT_PHASE_PERMILLE, ST_DEFAULT_DELAY_PERMILLE, ST_DEFAULT_MONO_DB, ST_DEFAULT_BALANCE_DB = 64, 587, 420, 40, 12


class StereoOpts(C.Structure):  # rg_stereo_opts
    _fields_ = [("block_frames", C.c_uint32), ("radius", C.c_uint32), ("phase_permille", C.c_uint32), ("delay_permille", C.c_uint32),
                ("mono_db", C.c_uint32), ("balance_db_limit", C.c_uint32)]


class StereoRecord(C.Structure):  # rg_stereo_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("block_frames", C.c_uint32),
        ("radius", C.c_uint32),
        ("blocks", C.c_uint32),
        ("active_blocks", C.c_uint32),
        ("neg_blocks", C.c_uint32),
        ("mono_blocks", C.c_uint32),
        ("lag", C.c_int32),
        ("anti_lag", C.c_int32),
        ("equal_frames", C.c_uint64),
        ("opposite_frames", C.c_uint64),
        ("zero_frames", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("ell", C.c_int64),
        ("err", C.c_int64),
        ("elr", C.c_int64),
        ("lag_sum", C.c_int64),
        ("anti_sum", C.c_int64),
        ("correlation", C.c_double),
        ("lag_correlation", C.c_double),
        ("anti_correlation", C.c_double),
        ("balance_db", C.c_double),
        ("side_db", C.c_double),
    ]


STEREO_SYMBOLS = [
    ("rg_stereo", _int, [_vp, _P(C.c_char_p), _sz, _P(StereoOpts), _P(StereoRecord), _P(C.c_int64)]),
    ("rg_stereo_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(StereoOpts), _vp, _sz, _P(StereoRecord), _P(C.c_int64)]),
    ("rg_stereo_kernel_shape", _int, [_u32, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_stereo_rate", _int, [_vp, _sz, _u64, _u32, _u32, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz), _P(_u64), _P(_u64)]),
]

# include/mp3rgain_amd_compare.h (null test of two tracks: lag rows around a hint, the pick, aligned moments per block)
(CMP_COMPLETE, CMP_IDENTICAL, CMP_SHIFTED, CMP_LENGTHS, CMP_INVERTED, CMP_NONFINITE, CMP_LOCKED, CMP_AT_EDGE, CMP_DRIFT, CMP_SAME_MASTER,
 CMP_DIFFERS, CMP_UNRELATED, CMP_RATE, CMP_NO_OVERLAP, CMP_NO_COARSE, CMP_CHANNELS_DIFFER, CMP_RAW) = (1 << k for k in range(17))
CMP_ALIGN_FINGERPRINT, CMP_ALIGN_HINT = 0, 1
CMP_MAX_CHANNELS, CMP_MAX_RADIUS, CMP_MAX_COARSE_RADIUS, CMP_MAX_SEGMENTS, CMP_MAX_BLOCK_FRAMES, CMP_MAX_HINT = 8, 2047, 2047, 16, 384000, 1 << 32
(CMP_DEFAULT_COARSE_RADIUS, CMP_DEFAULT_RADIUS, CMP_DEFAULT_SEGMENTS, CMP_DEFAULT_SEGMENT_FRAMES, CMP_DEFAULT_DRIFT_FRAMES,
 CMP_DEFAULT_LOCK_PERMILLE, CMP_DEFAULT_REQUANT_MILLILSB2) = 512, 1024, 4, 262144, 1, 606, 18156
CMP_NONE = (1 << 64) - 1  # first_diff: no sample differs


class ComparePair(C.Structure):  # rg_compare_pair
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("hint", C.c_int64)]


class CompareOpts(C.Structure):  # rg_compare_opts
    _fields_ = [("align", C.c_uint32), ("coarse_radius", C.c_uint32), ("radius", C.c_uint32), ("segments", C.c_uint32), ("segment_frames", C.c_uint32),
                ("block_frames", C.c_uint32), ("drift_frames", C.c_uint32), ("lock_permille", C.c_uint32), ("requant_millilsb2", C.c_uint32)]


class CompareBlock(C.Structure):  # rg_compare_block
    _fields_ = [("aa", C.c_int64), ("bb", C.c_int64), ("ab", C.c_int64), ("first_diff", C.c_uint64), ("equal", C.c_uint32), ("max_diff", C.c_uint32),
                ("frames", C.c_uint32), ("reserved", C.c_uint32)]


class CompareRecord(C.Structure):  # rg_compare_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("a", C.c_uint32),
        ("b", C.c_uint32),
        ("frames_a", C.c_uint64),
        ("frames_b", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format_a", C.c_uint32),
        ("format_b", C.c_uint32),
        ("dropped_a", C.c_uint32),
        ("dropped_b", C.c_uint32),
        ("block_frames", C.c_uint32),
        ("radius", C.c_uint32),
        ("segments", C.c_uint32),
        ("locked_segments", C.c_uint32),
        ("polarity", C.c_int32),
        ("max_diff", C.c_uint32),
        ("hint", C.c_int64),
        ("lag", C.c_int64),
        ("seg_lag_min", C.c_int64),
        ("seg_lag_max", C.c_int64),
        ("overlap", C.c_uint64),
        ("a_head", C.c_uint64),
        ("a_tail", C.c_uint64),
        ("b_head", C.c_uint64),
        ("b_tail", C.c_uint64),
        ("blocks", C.c_uint32),
        ("differing_blocks", C.c_uint32),
        ("worst_block", C.c_uint32),
        ("reserved", C.c_uint32),
        ("equal", C.c_uint64),
        ("first_diff", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("aa", C.c_int64),
        ("bb", C.c_int64),
        ("ab", C.c_int64),
        ("lock", C.c_double),
        ("gain_db", C.c_double),
        ("null_unity_db", C.c_double),
        ("null_db", C.c_double),
        ("residual_lsb2", C.c_double),
        ("worst_block_db", C.c_double),
        ("gain_min_db", C.c_double),
        ("gain_max_db", C.c_double),
    ]


COMPARE_SYMBOLS = [
    ("rg_compare_error", C.c_char_p, [_vp, _sz]),
    ("rg_compare", _int, [_vp, _P(C.c_char_p), _sz, _P(ComparePair), _sz, _P(CompareOpts), _P(CompareRecord), _P(CompareBlock), _sz, _P(C.c_int64)]),
    ("rg_compare_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _sz, _P(ComparePair), _P(CompareOpts), _vp, _sz, _P(CompareRecord), _P(CompareBlock), _sz,
                                _P(C.c_int64)]),
    ("rg_compare_kernel_shape", _int, [_u32, _u32, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_compare_rate", _int, [_vp, _sz, _sz, _u64, _u32, _P(CompareOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz), _P(_u64), _P(_u64)]),
]

# include/mp3rgain_amd_flacenc.h (FLAC encoder: LPC search, exact Rice sizing)
FLAC_ENC_DEFAULT_BLOCK, FLAC_ENC_DEFAULT_LPC, FLAC_ENC_MAX_LPC, FLAC_ENC_VERIFY = 4096, 8, 12, 1
FLAC_ENC_COMPLETE, FLAC_ENC_VERIFIED, FLAC_ENC_WRITTEN, FLAC_ENC_VERIFY_FAILED = 1, 2, 4, 8


class FlacEncodeOptions(C.Structure):  # rg_flac_encode_options
    _fields_ = [("struct_size", C.c_uint32), ("block_size", C.c_uint32), ("max_lpc_order", C.c_uint32), ("flags", C.c_uint32)]


class FlacEncodeRecord(C.Structure):  # rg_flac_encode_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("pcm_frames", C.c_uint64),
        ("flac_frames", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("bits_per_sample", C.c_uint32),
        ("block_size", C.c_uint32),
        ("min_frame_bytes", C.c_uint32),
        ("max_frame_bytes", C.c_uint32),
        ("pcm_bytes", C.c_uint64),
        ("stream_bytes", C.c_uint64),
        ("metadata_bytes", C.c_uint64),
        ("md5_pcm", C.c_uint8 * 16),
        ("md5_decoded", C.c_uint8 * 16),
    ]


FLACENC_SYMBOLS = [
    ("rg_flac_encode_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(_u32), _vp, _sz, _P(FlacEncodeOptions), _vp, _sz, _P(_u64), _P(FlacEncodeRecord)]),
    ("rg_flac_encode_files", _int, [_vp, _P(C.c_char_p), _P(C.c_char_p), _sz, _P(FlacEncodeOptions), _P(FlacEncodeRecord)]),
    ("rg_flac_encode_source_blocks", _int, [_vp, _sz, _vp, _sz, _P(_sz)]),
    ("rg_flac_encode_rate", _int, [_vp, _sz, _P(TrackDesc), _P(_u32), _vp, _sz, _P(FlacEncodeOptions), _u32, _P(_dbl), _P(_u64)]),
]

# include/mp3rgain_amd_clicks.h (clicks and glitches: the encoder's linear model per block, residual against the local median, events)
CK_COMPLETE, CK_SILENT, CK_NONFINITE, CK_CLICKS, CK_BURSTS, CK_TRUNCATED = (1 << k for k in range(6))
CK_KIND_CLICK, CK_KIND_BURST = 1, 2
CK_MAX_CHANNELS, CK_MAX_ORDER, CK_MAX_EVENTS = 8, 12, 256
(CK_DEFAULT_BLOCK, CK_DEFAULT_ORDER, CK_DEFAULT_RATIO_PERMILLE, CK_DEFAULT_FLOOR, CK_DEFAULT_GAP, CK_DEFAULT_MAX_WIDTH,
 CK_DEFAULT_MAX_EVENTS) = 1024, 8, 8371, 4, 16, 32, 16


class ClicksOpts(C.Structure):  # rg_clicks_opts
    _fields_ = [("block_samples", C.c_uint32), ("order", C.c_uint32), ("ratio_permille", C.c_uint32), ("floor", C.c_uint32), ("gap", C.c_uint32),
                ("max_width", C.c_uint32), ("max_events", C.c_uint32)]


class ClicksChannel(C.Structure):  # rg_clicks_channel
    _fields_ = [("flagged", C.c_uint32), ("clicks", C.c_uint32), ("bursts", C.c_uint32), ("widest", C.c_uint32), ("first_click", C.c_uint32),
                ("strongest_at", C.c_uint32), ("strongest_permille", C.c_uint32), ("fallback_blocks", C.c_uint32), ("median_max", C.c_uint32),
                ("reserved", C.c_uint32)]


class ClicksEvent(C.Structure):  # rg_clicks_event
    _fields_ = [("start", C.c_uint32), ("width", C.c_uint32), ("peak_at", C.c_uint32), ("strength_permille", C.c_uint32), ("channel", C.c_uint16),
                ("kind", C.c_uint16)]


class ClicksRecord(C.Structure):  # rg_clicks_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("block_samples", C.c_uint32),
        ("order", C.c_uint32),
        ("ratio_permille", C.c_uint32),
        ("floor", C.c_uint32),
        ("gap", C.c_uint32),
        ("max_width", C.c_uint32),
        ("max_events", C.c_uint32),
        ("listed", C.c_uint32),
        ("nonfinite", C.c_uint64),
        ("events", C.c_uint64),
        ("ch", ClicksChannel * CK_MAX_CHANNELS),
    ]


CLICKS_SYMBOLS = [
    ("rg_clicks", _int, [_vp, _P(C.c_char_p), _sz, _P(ClicksOpts), _P(ClicksRecord), _P(ClicksEvent)]),
    ("rg_clicks_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(ClicksOpts), _vp, _sz, _P(ClicksRecord), _P(ClicksEvent)]),
    ("rg_clicks_kernel_shape", _int, [_u32, _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_clicks_rate", _int, [_vp, _sz, _u64, _u32, _P(ClicksOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz), _P(_u64), _P(_u64)]),
]

# include/mp3rgain_amd_ancestry.h (lossy ancestry: an MP3 granule grid in PCM)
ANC_COMPLETE, ANC_MP3_GRID, ANC_MIDSIDE, ANC_NONFINITE, ANC_SHORT, ANC_SILENT = 1, 2, 4, 8, 16, 32
ANC_MAX_CHANNELS, ANC_MAX_VIEWS, ANC_ALIGNMENTS, ANC_VIEW_MID, ANC_VIEW_SIDE, ANC_NO_VIEW = 8, 10, 576, 8, 9, 0xFFFFFFFF
ANC_SEGMENTS, ANC_GRANULES = 16, 32
ANC_Z_MIN, ANC_ISO_MIN, ANC_ACTIVE_FLOOR = 19.01, 1.675, 0.00462963


class AncestryOpts(C.Structure):  # rg_ancestry_opts
    _fields_ = [("segments", C.c_uint32), ("granules", C.c_uint32), ("z_min", C.c_double), ("iso_min", C.c_double),
                ("active_floor", C.c_float), ("reserved", C.c_uint32)]


class AncestryView(C.Structure):  # rg_ancestry_view
    _fields_ = [
        ("ratio", C.c_double),
        ("second", C.c_double),
        ("p0", C.c_double),
        ("z", C.c_double),
        ("iso", C.c_double),
        ("small", C.c_uint64),
        ("active", C.c_uint64),
        ("active_total", C.c_uint64),
        ("offset", C.c_uint32),
        ("kind", C.c_uint32),
        ("flagged", C.c_uint32),
        ("nonfinite", C.c_uint32),
    ]


class AncestryRecord(C.Structure):  # rg_ancestry_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("views", C.c_uint32),
        ("grid_offset", C.c_uint32),
        ("segments", C.c_uint32),
        ("granules", C.c_uint32),
        ("best_view", C.c_uint32),
        ("reserved", C.c_uint32),
        ("z", C.c_double),
        ("iso", C.c_double),
        ("view", AncestryView * ANC_MAX_VIEWS),
    ]


ANCESTRY_SYMBOLS = [
    ("rg_ancestry", _int, [_vp, _P(C.c_char_p), _sz, _P(AncestryOpts), _P(AncestryRecord)]),
    ("rg_ancestry_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _P(AncestryOpts), _vp, _sz, _P(AncestryRecord), _P(_u64)]),
    ("rg_ancestry_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_ancestry_rate", _int, [_vp, _sz, _u64, _P(AncestryOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_sz), _P(_dbl)]),
]

# include/mp3rgain_amd_fingerprint.h (duplicate recordings: fingerprints and the pair match)
FP_SHORT, FP_RATE, FP_NONFINITE, FP_COMPLETE = 1, 2, 4, 8
FP_PAIR_COMPARED, FP_PAIR_MATCH, FP_PAIR_SKIPPED, FP_PAIR_PROBE_J = 1, 2, 4, 8
FP_MAX_CHANNELS, FP_FRAME, FP_HOP, FP_BANDS = 8, 4096, 512, 33
FP_BLOCK, FP_PROBES, FP_RADIUS, FP_MAX_BER_PERMILLE = 256, 8, 512, 316
FP_MAX_BLOCK, FP_MAX_PROBES, FP_MAX_RADIUS = 4096, 64, 2047


class FingerprintOpts(C.Structure):  # rg_fingerprint_opts
    _fields_ = [("block", C.c_uint32), ("probes", C.c_uint32), ("radius", C.c_uint32), ("max_ber_permille", C.c_uint32)]


class FingerprintRecord(C.Structure):  # rg_fingerprint_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("fp_frames", C.c_uint32),
        ("codes", C.c_uint32),
        ("nonfinite_frames", C.c_uint32),
        ("group", C.c_uint32),
        ("matches", C.c_uint32),
        ("reserved", C.c_uint32),
        ("codes_at", C.c_uint64),
        ("frames_at", C.c_uint64),
    ]


class FingerprintPairRecord(C.Structure):  # rg_fingerprint_pair_record
    _fields_ = [("errors", C.c_uint32), ("bits", C.c_uint32), ("lag", C.c_int32), ("flags", C.c_uint32)]


class FingerprintPair(C.Structure):  # rg_fingerprint_pair
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("errors", C.c_uint32), ("bits", C.c_uint32), ("lag", C.c_int32), ("flags", C.c_uint32)]


FINGERPRINT_SYMBOLS = [
    ("rg_fingerprint_edges", _int, [_u32, _P(_u32)]),
    ("rg_same_recording", _int, [_vp, _P(C.c_char_p), _sz, _P(FingerprintOpts), _P(FingerprintRecord), _P(FingerprintPair), _sz, _P(_sz),
                                 _P(_u32), _sz]),
    ("rg_fingerprint_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _vp, _sz, _P(FingerprintRecord), _P(_u32), _P(C.c_float)]),
    ("rg_fingerprint_match_codes", _int, [_vp, _int, _sz, _P(_u32), _P(_u32), _P(_u32), _P(FingerprintOpts), _P(FingerprintPairRecord)]),
    ("rg_fingerprint_groups", _sz, [_sz, _P(FingerprintPairRecord), _P(_u32), _P(_u32)]),
    ("rg_fingerprint_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_fingerprint_rate", _int, [_vp, _sz, _u64, _P(FingerprintOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl),
                                   _P(_sz)]),
]

# include/mp3rgain_amd_tempo.h (tempo and beat grid: the onset curve and its windowed autocorrelation)
TEMPO_SHORT, TEMPO_RATE, TEMPO_NONFINITE, TEMPO_COMPLETE, TEMPO_RANGE, TEMPO_NONE = 1, 2, 4, 8, 16, 32
TEMPO_MAX_CHANNELS, TEMPO_FRAME, TEMPO_HOP, TEMPO_BANDS = 8, 4096, 512, 32
TEMPO_WINDOW, TEMPO_WINDOW_HOP, TEMPO_MIN_BPM = 1024, 256, 80
TEMPO_MIN_WINDOW, TEMPO_MAX_WINDOW, TEMPO_MAX_HARMONICS, TEMPO_ONSET_MAX = 32, 1024, 8, 1023
TEMPO_BEAT_BIAS = 4120


class TempoOpts(C.Structure):  # rg_tempo_opts
    _fields_ = [("window", C.c_uint32), ("hop", C.c_uint32), ("min_bpm", C.c_uint32)]


class TempoRecord(C.Structure):  # rg_tempo_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("onsets", C.c_uint32),
        ("windows", C.c_uint32),
        ("period16", C.c_uint32),
        ("harmonics", C.c_uint32),
        ("bpm_milli", C.c_uint32),
        ("confidence_permille", C.c_uint32),
        ("stable_permille", C.c_uint32),
        ("first_beat", C.c_uint32),
        ("nonfinite_frames", C.c_uint32),
        ("band_frames", C.c_uint32),
        ("onsets_at", C.c_uint64),
    ]


TEMPO_SYMBOLS = [
    ("rg_tempo_bands", _int, [_u32, _P(_u32)]),
    ("rg_tempo", _int, [_vp, _P(C.c_char_p), _sz, _P(TempoOpts), _P(TempoRecord), _P(C.c_uint16), _sz]),
    ("rg_tempo_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _vp, _sz, _P(TempoOpts), _P(TempoRecord), _P(C.c_uint16), _P(C.c_float)]),
    ("rg_tempo_from_onsets", _int, [_vp, _int, _sz, _P(_u32), _P(_u32), _P(C.c_uint16), _P(TempoOpts), _P(TempoRecord), _P(C.c_int64)]),
    ("rg_tempo_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_tempo_rate", _int, [_vp, _sz, _u64, _P(TempoOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl),
                             _P(_sz)]),
]

# include/mp3rgain_amd_key.h (musical key: the decimated chromagram and the key-profile match)
KEY_SHORT, KEY_RATE, KEY_NONFINITE, KEY_COMPLETE, KEY_NONE = 1, 2, 4, 8, 16
KEY_MAX_CHANNELS, KEY_FRAME, KEY_HOP, KEY_BANDS, KEY_CHROMA, KEY_RANGE = 8, 4096, 512, 60, 12, 160
KEY_TARGET_RATE, KEY_MAX_DECIM, KEY_TAPS_PER_DECIM = 5000, 80, 16
KEY_SEGMENT, KEY_MIN_SEGMENT, KEY_MAX_SEGMENT, KEY_ROW_MAX = 128, 8, 4096, 800


class KeyOpts(C.Structure):  # rg_key_opts
    _fields_ = [("segment", C.c_uint32)]


class KeyRecord(C.Structure):  # rg_key_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("decim", C.c_uint32),
        ("decimated", C.c_uint32),
        ("rows", C.c_uint32),
        ("silent_rows", C.c_uint32),
        ("nonfinite_frames", C.c_uint32),
        ("key", C.c_uint32),
        ("tonic", C.c_uint32),
        ("mode", C.c_uint32),
        ("correlation_permille", C.c_uint32),
        ("margin_permille", C.c_uint32),
        ("segments", C.c_uint32),
        ("stable_permille", C.c_uint32),
        ("chroma_at", C.c_uint64),
    ]


KEY_SYMBOLS = [
    ("rg_key_bands", _int, [_u32, _P(_u32), _P(_u32)]),
    ("rg_key_filter", _int, [_u32, _P(C.c_float)]),
    ("rg_key", _int, [_vp, _P(C.c_char_p), _sz, _P(KeyOpts), _P(KeyRecord), _P(C.c_uint16), _sz]),
    ("rg_key_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _vp, _sz, _P(KeyOpts), _P(KeyRecord), _P(C.c_float), _P(C.c_float), _P(C.c_uint16)]),
    ("rg_key_from_chroma", _int, [_vp, _int, _sz, _P(_u32), _P(C.c_uint16), _P(KeyOpts), _P(KeyRecord)]),
    ("rg_key_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_key_rate", _int, [_vp, _sz, _u64, _P(KeyOpts), _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz)]),
]

# include/mp3rgain_amd_resample.h (duplicates across sample rates: the rational resampler and the cross-rate fingerprint)
RS_SHORT, RS_RATE = 1, 2
RS_RATE_OUT, RS_MAX_PHASES, RS_MAX_RATIO, RS_MIN_RATE, RS_HALF_PER_W, RS_MAX_CHANNELS = 11025, 441, 32, 8000, 8, 8
XR_BLOCK, XR_PROBES, XR_RADIUS, XR_MAX_BER_PERMILLE = 64, 8, 128, 303


class ResampleRecord(C.Structure):  # rg_resample_result
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("format", C.c_uint32),
        ("up", C.c_uint32),
        ("down", C.c_uint32),
        ("taps", C.c_uint32),
        ("resampled", C.c_uint32),
        ("reserved", C.c_uint32),
        ("y_at", C.c_uint64),
    ]


class XrateRecord(C.Structure):  # rg_xrate_result
    _fields_ = FingerprintRecord._fields_ + [
        ("up", C.c_uint32),
        ("down", C.c_uint32),
        ("resampled", C.c_uint32),
        ("reserved2", C.c_uint32),
        ("y_at", C.c_uint64),
    ]


RESAMPLE_SYMBOLS = [
    ("rg_resample_plan", _int, [_u32, _P(_u32), _P(_u32), _P(_u32)]),
    ("rg_resample_filter", _int, [_u32, _u32, _P(C.c_float)]),
    ("rg_resample_window", _int, [_u32, _u64, _P(_u64), _P(_u32)]),
    ("rg_resample_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _vp, _sz, _P(ResampleRecord), _P(C.c_float)]),
    ("rg_xrate_fingerprint_arena", _int, [_vp, _int, _sz, _P(TrackDesc), _vp, _sz, _P(XrateRecord), _P(_u32), _P(C.c_float), _P(C.c_float)]),
    ("rg_same_recording_xrate", _int, [_vp, _P(C.c_char_p), _sz, _P(FingerprintOpts), _P(XrateRecord), _P(FingerprintPair), _sz, _P(_sz),
                                       _P(_u32), _sz]),
    ("rg_resample_kernel_shape", _int, [_P(_u32), _P(_u32), _P(_u32)]),
    ("rg_resample_rate", _int, [_vp, _sz, _u64, _u32, _sz, _u32, _u32, _dbl, _P(_dbl), _P(_dbl), _P(_dbl), _P(_sz)]),
]

# rg_node_backend (include/mp3rgain_amd_node.h): a table of per-device functions
NODE_OPEN = C.CFUNCTYPE(_vp, _int, _vp)
NODE_CLOSE = C.CFUNCTYPE(None, _vp, _vp)
NODE_ALBUM_BEGIN = C.CFUNCTYPE(_int, _vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(_sz), _vp)
NODE_ALBUM_PACK = C.CFUNCTYPE(_int, _vp, _P(_u32), _vp)
NODE_TRACKS = C.CFUNCTYPE(_int, _vp, _P(C.c_char_p), _sz, _i32, _P(TrackResult), _P(_i32), _vp)
NODE_TRACKS_ERROR = C.CFUNCTYPE(_vp, _vp, _sz, _vp)  # const char *: the callee keeps the bytes alive
NODE_LAST_ERROR = C.CFUNCTYPE(_vp, _vp, _vp)


class NodeBackend(C.Structure):
    _fields_ = [("open", NODE_OPEN), ("close", NODE_CLOSE), ("album_begin", NODE_ALBUM_BEGIN), ("album_pack", NODE_ALBUM_PACK),
                ("tracks", NODE_TRACKS), ("tracks_error", NODE_TRACKS_ERROR), ("last_error", NODE_LAST_ERROR), ("user", _vp)]


_lib = None


def load():
    """Load libmp3rgain_amd.so from the package directory (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C mp3rgain_amd/csrc). There is no fallback path."
            )
        # When PyTorch shares the process (tests, bench.py), let it bring its bundled HIP runtime in
        # first: two HIP runtimes in one process cannot both own the device.
        import importlib.util
        import sys

        # A process that will never import torch (the command line, `python -m mp3rgain_amd`) says so with
        # MP3RGAIN_AMD_STANDALONE=1 and saves the 1.5 s that import costs: the library then runs on the system's HIP runtime.
        import os

        standalone = os.environ.get("MP3RGAIN_AMD_STANDALONE") == "1"
        if not standalone and "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
        L = C.CDLL(str(LIB_PATH))
        for name, res, args in SYMBOLS + R128_SYMBOLS + RIP_SYMBOLS + STATS_SYMBOLS + SPECTRUM_SYMBOLS + DR_SYMBOLS + STEREO_SYMBOLS + COMPARE_SYMBOLS + CLICKS_SYMBOLS + FLACENC_SYMBOLS + ANCESTRY_SYMBOLS + FINGERPRINT_SYMBOLS + TEMPO_SYMBOLS + KEY_SYMBOLS + RESAMPLE_SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib
