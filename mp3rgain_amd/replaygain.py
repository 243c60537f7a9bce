"""Host-side mirror of mp3rgain's `replaygain` module on decoded PCM, over the C ABI.

Names, fields, argument meaning and error behaviour follow the reference
(src/replaygain.rs, v1.5.0):

  REPLAYGAIN_REFERENCE_DB                          :37
  AudioFileType {Mp3, Aac}                         :48-53
  ReplayGainResult {loudness_db, gain_db, peak, sample_rate, file_type} + gain_steps()   :57-75
  AlbumGainResult {tracks, album_loudness_db, album_gain_db, album_peak} + album_gain_steps()  :79-95
  analyze_track / analyze_album                    :929-941 / :1033-1074
  PeakAmplitudeResult / find_peak_amplitude        :1125-1132 / :1140-1249
  is_available                                     :1119-1121

The reference's functions take a file path and decode with symphonia; the decoder is outside
this path, so the functions here take a `PcmTrack` -- what the
reference's decode loop hands to process_audio_buffer, as whole planar channels.  All
arithmetic happens in libmp3rgain_amd.so on the GPU; this file is plumbing.
"""
from __future__ import annotations

import ctypes as C
import os
import time
import enum
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _capi

REPLAYGAIN_REFERENCE_DB = 89.0
GAIN_STEP_DB = 1.5
SUPPORTED_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000)


class ReplayGainError(RuntimeError):
    """The anyhow::Error of the reference: carries the library's message."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class AudioFileType(enum.IntEnum):
    Mp3 = 0
    Aac = 1


@dataclass
class ReplayGainResult:
    loudness_db: float
    gain_db: float
    peak: float
    sample_rate: int
    file_type: AudioFileType = AudioFileType.Mp3
    windows: int = 0
    flags: int = 0  # RG_TRACK_FLAG_*: 1 = non-finite samples in the track, 2 = a window variant 2 could not resolve

    def gain_steps(self) -> int:
        return _capi.load().rg_gain_steps(self.gain_db)


@dataclass
class AlbumGainResult:
    tracks: List[ReplayGainResult]
    album_loudness_db: float
    album_gain_db: float
    album_peak: float

    def album_gain_steps(self) -> int:
        return _capi.load().rg_gain_steps(self.album_gain_db)


@dataclass
class PeakAmplitudeResult:
    peak: float
    peak_pcm: float
    sample_rate: int


R128_REFERENCE_LUFS = -18.0


@dataclass
class R128Dynamics:
    """Loudness range (EBU Tech 3342) and the momentary / short-term maxima of a track or an album (rg_r128_dynamics)."""

    loudness_range_lu: float
    range_low_lufs: float
    range_high_lufs: float
    max_momentary_lufs: float
    max_short_term_lufs: float
    st_blocks: int = 0
    st_blocks_gated: int = 0


@dataclass
class R128Result:
    """EBU R 128 / ReplayGain 2.0 result of one track (rg_r128_track_result, include/mp3rgain_amd_r128.h).  `peak` is what
    the gain-step and clip-limiting code downstream reads: the true peak when it was asked for, else the sample peak."""

    loudness_lufs: float
    gain_db: float
    sample_peak: float
    true_peak: float  # NaN when not asked for
    sample_rate: int
    blocks: int = 0
    blocks_gated: int = 0
    flags: int = 0
    file_type: AudioFileType = AudioFileType.Mp3
    dynamics: Optional[R128Dynamics] = None  # asked for with dynamics=True

    @property
    def peak(self) -> float:
        return self.sample_peak if self.true_peak != self.true_peak else self.true_peak

    def gain_steps(self) -> int:
        return _capi.load().rg_gain_steps(self.gain_db)


@dataclass
class R128AlbumResult:
    tracks: List[R128Result]
    loudness_lufs: float
    gain_db: float
    sample_peak: float
    true_peak: float
    blocks: int = 0
    blocks_gated: int = 0
    dynamics: Optional[R128Dynamics] = None  # asked for with dynamics=True

    @property
    def peak(self) -> float:
        return self.sample_peak if self.true_peak != self.true_peak else self.true_peak

    def album_gain_steps(self) -> int:
        return _capi.load().rg_gain_steps(self.gain_db)


def r128_design_info(sample_rate: int) -> dict:
    """The K-weighting biquads, hop and true-peak factor of one rate (rg_r128_design_info; host only)."""
    b1, a1, b2, a2 = ((C.c_double * 3)() for _ in range(4))
    hop, fac = C.c_uint32(), C.c_uint32()
    rc = _capi.load().rg_r128_design_info(sample_rate, b1, a1, b2, a2, C.byref(hop), C.byref(fac))
    if rc != _capi.RG_OK:
        raise ReplayGainError(rc, f"Unsupported sample rate: {sample_rate} Hz. Supported rates: 8000 to 384000")
    return {"b1": list(b1), "a1": list(a1), "b2": list(b2), "a2": list(a2), "hop": hop.value, "tp_factor": fac.value}


_NP_FMT = {
    np.dtype(np.float32): _capi.FMT_F32_PLANAR,
    np.dtype(np.int16): _capi.FMT_S16_PLANAR,
    np.dtype(np.int32): _capi.FMT_S32_PLANAR,
}


def rip_checksums_arena(ctx, route: int, descs, flags, arena):
    """rg_rip_checksums_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> [RipRecord]."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    fl = None if flags is None else (C.c_uint32 * max(1, n))(*[int(f) for f in flags])
    out = (_capi.RipRecord * max(1, n))()
    rc = L.rg_rip_checksums_arena(ctx, int(route), n, d, fl, arena.ctypes.data if arena.size else None, arena.size, out)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n])


def rip_kernel_shape():
    """rg_rip_kernel_shape -> (chunk_frames, tile_frames, fold_lanes)."""
    c, t, f = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _capi.load().rg_rip_kernel_shape(C.byref(c), C.byref(t), C.byref(f))
    return c.value, t.value, f.value


def rip_offsets_arena(ctx, route: int, descs, flags, radius: int, arena, want=(True, True)):
    """rg_rip_offsets_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> (arv1, arv2), uint32
    arrays [n, 2 radius + 1] indexed [t][o + radius]; `want` says which of the two are computed (the other is None)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    fl = None if flags is None else (C.c_uint32 * max(1, n))(*[int(f) for f in flags])
    width = 2 * max(0, min(int(radius), _capi.RIP_OFFSET_MAX)) + 1
    tabs = [np.zeros((n, width), dtype=np.uint32) if w else None for w in want]
    ptr = [t.ctypes.data_as(C.POINTER(C.c_uint32)) if t is not None else None for t in tabs]
    rc = L.rg_rip_offsets_arena(ctx, int(route), n, d, fl, int(radius), arena.ctypes.data if arena.size else None, arena.size, ptr[0], ptr[1])
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return tabs[0], tabs[1]


def rip_offsets_kernel_shape():
    """rg_rip_offsets_kernel_shape -> (tile_frames, block_lanes)."""
    t, b = C.c_uint32(), C.c_uint32()
    _capi.load().rg_rip_offsets_kernel_shape(C.byref(t), C.byref(b))
    return t.value, b.value


def _stats_opts(min_clip_run, min_zero_run):
    """rg_pcm_stats_opts, or NULL (the header's defaults) when both are None."""
    if min_clip_run is None and min_zero_run is None:
        return None
    return C.byref(_capi.PcmStatsOpts(_capi.STATS_MIN_CLIP_RUN if min_clip_run is None else int(min_clip_run),
                                      _capi.STATS_MIN_ZERO_RUN if min_zero_run is None else int(min_zero_run)))


def pcm_stats_arena(ctx, route: int, descs, bits, arena, min_clip_run=None, min_zero_run=None):
    """rg_pcm_stats_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> [PcmStatsRecord].  `bits`:
    one entry per track, or None (the container's width everywhere); both run lengths None = the header's defaults."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    b = None if bits is None else (C.c_uint32 * max(1, n))(*[int(x) for x in bits])
    out = (_capi.PcmStatsRecord * max(1, n))()
    rc = L.rg_pcm_stats_arena(ctx, int(route), n, d, b, _stats_opts(min_clip_run, min_zero_run), arena.ctypes.data if arena.size else None,
                              arena.size, out)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n])


def pcm_stats_kernel_shape():
    """rg_pcm_stats_kernel_shape -> (chunk_samples, tile_samples, fold_lanes)."""
    c, t, f = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _capi.load().rg_pcm_stats_kernel_shape(C.byref(c), C.byref(t), C.byref(f))
    return c.value, t.value, f.value


@dataclass
class ChannelStats:
    """One channel of a PcmStats (rg_pcm_stats_channel, include/mp3rgain_amd_stats.h)."""
    min: float               # over the stored values (the finite ones for float)
    max: float
    sum: int                 # of the stored values; float: of llrint(clamp(x, -256, 256) * 2^23)
    or_mask: int
    effective_bits: int
    clipped: int             # samples at full scale
    clip_runs: int           # stretches of at least min_clip_run of them
    longest_clip_run: int
    first_clip_run: int      # first sample of the first counted stretch; `frames` when there is none
    zeros: int
    lead_zeros: int
    trail_zeros: int
    zero_runs: int           # zero stretches of at least min_zero_run that touch neither end
    longest_zero_run: int
    nonfinite: int
    frames: int = 0
    full_scale: float = 1.0  # 2^(W-1) for the integer formats, 1.0 for float: what min and max are relative to
    sum_scale: float = 1.0   # 2^(W-1) for the integer formats, 2^23 for float

    @property
    def dc_offset(self) -> float:
        """The mean sample value relative to full scale."""
        return self.sum / self.frames / self.sum_scale if self.frames else 0.0

    @property
    def peak(self) -> float:
        """max(|min|, |max|) relative to full scale."""
        return max(abs(self.min), abs(self.max)) / self.full_scale


@dataclass
class PcmStats:
    """One file of Analyzer.pcm_stats (rg_pcm_stats_result): what is wrong with the audio itself."""
    frames: int
    sample_rate: int
    format: int              # rg_sample_format of the planes that were scanned
    bits: int                # 0 for float
    dropped_frames: int
    lead_silence_frames: int
    trail_silence_frames: int
    flags: int
    channels: list           # [ChannelStats]
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    @property
    def clipped(self) -> bool:
        return bool(self.flags & _capi.STATS_CLIPPED)

    @property
    def dropout(self) -> bool:
        return bool(self.flags & _capi.STATS_DROPOUT)

    @property
    def padded(self) -> bool:
        return bool(self.flags & _capi.STATS_PADDED)

    @property
    def nonfinite(self) -> bool:
        return bool(self.flags & _capi.STATS_NONFINITE)

    @property
    def silent(self) -> bool:
        return bool(self.flags & _capi.STATS_SILENT)

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.STATS_COMPLETE)

    @property
    def effective_bits(self) -> int:
        return max((c.effective_bits for c in self.channels), default=0)

    @property
    def dc_offset(self) -> float:
        """The largest DC offset of the channels, by magnitude."""
        return max((c.dc_offset for c in self.channels), key=abs, default=0.0)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        names = (("clipped", self.clipped), ("dropout", self.dropout), ("padded", self.padded), ("nonfinite", self.nonfinite),
                 ("silent", self.silent), ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]


def pcm_stats_from_record(r, error=None) -> PcmStats:
    """A PcmStats from an rg_pcm_stats_result."""
    w = 16 if r.format == _capi.FMT_S16_PLANAR else 32
    is_float = r.format == _capi.FMT_F32_PLANAR
    full, scale = (1.0, float(1 << 23)) if is_float else (float(1 << (w - 1)),) * 2
    ch = []
    for k in range(int(r.channels)):
        c = r.ch[k]
        ch.append(ChannelStats(float(c.min), float(c.max), int(c.sum), int(c.or_mask), int(c.effective_bits), int(c.clipped), int(c.clip_runs),
                               int(c.longest_clip_run), int(c.first_clip_run), int(c.zeros), int(c.lead_zeros), int(c.trail_zeros),
                               int(c.zero_runs), int(c.longest_zero_run), int(c.nonfinite), int(r.frames), full, scale))
    return PcmStats(int(r.frames), int(r.sample_rate), int(r.format), int(r.bits), int(r.dropped_frames), int(r.lead_silence_frames),
                    int(r.trail_silence_frames), int(r.flags), ch, error)


def _dr_opts(block_frames, top_permille):
    """rg_dr_opts, or NULL (the header's defaults) when both are None."""
    if block_frames is None and top_permille is None:
        return None
    return C.byref(_capi.DrOpts(0 if block_frames is None else int(block_frames),
                                _capi.DR_TOP_PERMILLE if top_permille is None else int(top_permille)))


def dr_arena(ctx, route: int, descs, arena, block_frames=None, top_permille=None):
    """rg_dr_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> [DrRecord].  Both options None =
    the header's defaults (3-second blocks, the loudest 200 per mille)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.DrRecord * max(1, n))()
    rc = L.rg_dr_arena(ctx, int(route), n, d, _dr_opts(block_frames, top_permille), arena.ctypes.data if arena.size else None, arena.size, out)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n])


def dr_kernel_shape(fmt: int):
    """rg_dr_kernel_shape of one rg_sample_format -> (step_samples, piece_samples, fold_lanes, select_bins)."""
    c, t, f, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = _capi.load().rg_dr_kernel_shape(int(fmt), C.byref(c), C.byref(t), C.byref(f), C.byref(b))
    if rc != 0:
        raise ReplayGainError(rc, f"rg_dr_kernel_shape: format {fmt}")
    return c.value, t.value, f.value, b.value


@dataclass
class ChannelDynamicRange:
    """One channel of a DynamicRange (rg_dr_channel, include/mp3rgain_amd_dr.h)."""
    dr: float                # 20 log10((peak2 / s) / sqrt(top_ms)); 0 when either is 0
    peak_db: float           # -inf for a channel of zeros
    rms_db: float
    top_ms: float            # the mean of the loudest blocks' mean squares (with the factor 2)
    mean_square: float
    peak: int                # in units of q
    peak2: int               # the second-highest block peak
    blocks: int
    top_blocks: int
    nonfinite: int


@dataclass
class DynamicRange:
    """One file of Analyzer.dynamic_range (rg_dr_result).  The figure follows the published description of the TT DR meter
    and is a convention of include/mp3rgain_amd_dr.h: nobody has checked it against the TT meter or foobar2000."""
    frames: int
    sample_rate: int
    format: int              # rg_sample_format of the planes that were scanned
    dropped_frames: int
    block_frames: int
    flags: int
    dr: int                  # llrint(dr_mean)
    dr_mean: float
    peak_db: float
    rms_db: float
    channels: list           # [ChannelDynamicRange]
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.DR_COMPLETE)

    @property
    def silent(self) -> bool:
        return bool(self.flags & _capi.DR_SILENT)

    @property
    def nonfinite(self) -> bool:
        return bool(self.flags & _capi.DR_NONFINITE)

    @property
    def short(self) -> bool:
        return bool(self.flags & _capi.DR_SHORT)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        names = (("silent", self.silent), ("short", self.short), ("nonfinite", self.nonfinite),
                 ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]


def dynamic_range_from_record(r, error=None) -> DynamicRange:
    """A DynamicRange from an rg_dr_result."""
    ch = []
    for k in range(int(r.channels)):
        c = r.ch[k]
        ch.append(ChannelDynamicRange(float(c.dr), float(c.peak_db), float(c.rms_db), float(c.top_ms), float(c.mean_square), int(c.peak),
                                      int(c.peak2), int(c.blocks), int(c.top_blocks), int(c.nonfinite)))
    return DynamicRange(int(r.frames), int(r.sample_rate), int(r.format), int(r.dropped_frames), int(r.block_frames), int(r.flags), int(r.dr),
                        float(r.dr_mean), float(r.peak_db), float(r.rms_db), ch, error)


def album_dr(records) -> Optional[int]:
    """The album's figure: llrint (half to even) of the mean of the integer `dr` of the tracks that are complete and have no
    error; None when there is no such track.  A convention, like the rest of include/mp3rgain_amd_dr.h."""
    vals = [r.dr for r in records if r.error is None and r.complete]
    return int(round(sum(vals) / len(vals))) if vals else None


def _stereo_opts(radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit):
    """rg_stereo_opts, or NULL (the header's defaults) when all are None; a None field is its default."""
    if all(v is None for v in (radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit)):
        return None
    pick = lambda v, d: d if v is None else int(v)  # noqa: E731
    return C.byref(_capi.StereoOpts(pick(block_frames, 0), pick(radius, _capi.ST_DEFAULT_RADIUS), pick(phase_permille, _capi.ST_DEFAULT_PHASE_PERMILLE),
                                    pick(delay_permille, _capi.ST_DEFAULT_DELAY_PERMILLE), pick(mono_db, _capi.ST_DEFAULT_MONO_DB),
                                    pick(balance_db_limit, _capi.ST_DEFAULT_BALANCE_DB)))


def _stereo_rows(n, radius, wanted):
    """The caller's lag sums: (an int64 array of n rows of 2 * radius + 1, its pointer), or (None, NULL) when not wanted."""
    if not wanted:
        return None, None
    r = _capi.ST_DEFAULT_RADIUS if radius is None else int(radius)
    rows = np.zeros((max(1, n), 2 * max(0, r) + 1), dtype=np.int64)
    return rows, rows.ctypes.data_as(C.POINTER(C.c_int64))


def stereo_arena(ctx, route: int, descs, arena, radius=None, block_frames=None, phase_permille=None, delay_permille=None, mono_db=None,
                 balance_db_limit=None, lag_sums=False):
    """rg_stereo_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> [StereoRecord], or with
    `lag_sums` ([StereoRecord], int64 array of one row of 2 * radius + 1 sums per track).  Options None = the header's defaults."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.StereoRecord * max(1, n))()
    rows, rows_p = _stereo_rows(n, radius, lag_sums)
    rc = L.rg_stereo_arena(ctx, int(route), n, d, _stereo_opts(radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit),
                           arena.ctypes.data if arena.size else None, arena.size, out, rows_p)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return (list(out[:n]), rows[:n]) if lag_sums else list(out[:n])


def _flac_encode_opts(block_size, max_lpc_order, verify=True):
    """rg_flac_encode_options, or NULL (the header's defaults) when nothing departs from them."""
    if block_size is None and max_lpc_order is None and verify:
        return None
    return C.byref(_capi.FlacEncodeOptions(C.sizeof(_capi.FlacEncodeOptions), 0 if block_size is None else int(block_size),
                                           _capi.FLAC_ENC_DEFAULT_LPC if max_lpc_order is None else int(max_lpc_order),
                                           _capi.FLAC_ENC_VERIFY if verify else 0))


@dataclass
class FlacEncoded:
    """One file of Analyzer.encode_flac (rg_flac_encode_result)."""
    pcm_frames: int
    flac_frames: int
    dropped_frames: int      # FLAC frames of the source that did not decode
    sample_rate: int
    channels: int
    bits_per_sample: int
    block_size: int
    min_frame_bytes: int
    max_frame_bytes: int
    pcm_bytes: int
    stream_bytes: int
    metadata_bytes: int
    md5_pcm: bytes
    md5_decoded: bytes
    flags: int
    error: Optional[Exception] = None

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.FLAC_ENC_COMPLETE)

    @property
    def verified(self) -> bool:
        return bool(self.flags & _capi.FLAC_ENC_VERIFIED)

    @property
    def written(self) -> bool:
        return bool(self.flags & _capi.FLAC_ENC_WRITTEN)

    @property
    def verify_failed(self) -> bool:
        return bool(self.flags & _capi.FLAC_ENC_VERIFY_FAILED)

    @property
    def ratio(self) -> float:
        """Stream bytes over PCM bytes (0 for a file without audio)."""
        return self.stream_bytes / self.pcm_bytes if self.pcm_bytes else 0.0


def flac_encode_arena(ctx, route: int, descs, bps, arena, block_size=None, max_lpc_order=None):
    """rg_flac_encode_arena without an Analyzer: route 0 is the serial host twin and takes ctx = None.  The tracks `descs`
    describe in the host arena `arena` (left-justified integer planes of `bps` [int] bits) -> ([the FLAC stream of each track
    as bytes], [FlacEncodeRecord], the offsets as the call set them)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    b = (C.c_uint32 * max(1, n))(*[int(v) for v in bps])
    res = (_capi.FlacEncodeRecord * max(1, n))()
    offsets = (C.c_uint64 * (n + 1))()
    opts = _flac_encode_opts(block_size, max_lpc_order)
    out = np.zeros(0, dtype=np.uint8)
    for _ in range(2):  # the first call, into nothing, says how much the streams take
        rc = L.rg_flac_encode_arena(ctx, int(route), n, d, b, arena.ctypes.data if arena.size else None, arena.size, opts,
                                    out.ctypes.data if out.size else None, out.size, offsets, res)
        if rc == 0 or int(offsets[n]) <= out.size:
            break
        out = np.zeros(int(offsets[n]), dtype=np.uint8)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    offs = [int(v) for v in offsets]
    return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)], list(res[:n]), offs


def stereo_kernel_shape(fmt: int):
    """rg_stereo_kernel_shape of one rg_sample_format -> (piece_samples, tile_frames, strip_frames, lag_group, lds_bytes)."""
    v = [C.c_uint32() for _ in range(5)]
    rc = _capi.load().rg_stereo_kernel_shape(int(fmt), *[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, f"rg_stereo_kernel_shape: format {fmt}")
    return tuple(x.value for x in v)


_STEREO_FIELDS = ("frames", "sample_rate", "channels", "format", "dropped_frames", "block_frames", "radius", "flags", "blocks", "active_blocks",
                  "neg_blocks", "mono_blocks", "lag", "anti_lag", "equal_frames", "opposite_frames", "zero_frames", "nonfinite", "ell", "err", "elr",
                  "lag_sum", "anti_sum", "correlation", "lag_correlation", "anti_correlation", "balance_db", "side_db")


@dataclass
class StereoImage:
    """One file of Analyzer.stereo (rg_stereo_result): how channels 0 and 1 relate.  The definitions are a convention of
    include/mp3rgain_amd_stereo.h, tried on synthetic material only and held to no other tool."""
    frames: int
    sample_rate: int
    channels: int
    format: int              # rg_sample_format of the planes that were scanned
    dropped_frames: int
    block_frames: int
    radius: int
    flags: int
    blocks: int
    active_blocks: int
    neg_blocks: int
    mono_blocks: int
    lag: int                 # the lag with the largest sum; positive = the right channel is late
    anti_lag: int            # the lag with the smallest sum
    equal_frames: int
    opposite_frames: int
    zero_frames: int
    nonfinite: int
    ell: int
    err: int
    elr: int
    lag_sum: int
    anti_sum: int
    correlation: float
    lag_correlation: float
    anti_correlation: float
    balance_db: float        # +inf: all left, -inf: all right
    side_db: float           # -inf: no side signal, +inf: the mono sum cancels
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    def _has(self, bit) -> bool:
        return bool(self.flags & bit)

    @property
    def complete(self) -> bool:
        return self._has(_capi.ST_COMPLETE)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["stereo"] when there is nothing to report."""
        names = (("mono file", _capi.ST_MONO), ("silent", _capi.ST_SILENT), ("dual mono", _capi.ST_DUAL_MONO),
                 ("inverted copy", _capi.ST_INVERTED_COPY), ("out of phase", _capi.ST_OUT_OF_PHASE), ("near mono", _capi.ST_NEAR_MONO),
                 ("one-sided", _capi.ST_ONE_SIDED), ("delayed", _capi.ST_DELAYED), ("nonfinite", _capi.ST_NONFINITE),
                 ("more channels", _capi.ST_MORE_CHANNELS))
        words = [n for n, bit in names if self._has(bit)]
        if self.error is None and not self.complete:
            words.append("incomplete")
        return words or ["stereo"]


def stereo_from_record(r, error=None) -> StereoImage:
    """A StereoImage from an rg_stereo_result."""
    return StereoImage(*[(float if f in ("correlation", "lag_correlation", "anti_correlation", "balance_db", "side_db") else int)(getattr(r, f))
                         for f in _STEREO_FIELDS], error)


_COMPARE_OPTS = ("align", "coarse_radius", "radius", "segments", "segment_frames", "block_frames", "drift_frames", "lock_permille", "requant_millilsb2")


def _compare_opts(**given):
    """(rg_compare_opts with a None field at its default, the pointer to pass: NULL when all are None)."""
    defaults = dict(align=_capi.CMP_ALIGN_FINGERPRINT, coarse_radius=_capi.CMP_DEFAULT_COARSE_RADIUS, radius=_capi.CMP_DEFAULT_RADIUS,
                    segments=_capi.CMP_DEFAULT_SEGMENTS, segment_frames=_capi.CMP_DEFAULT_SEGMENT_FRAMES, block_frames=0,
                    drift_frames=_capi.CMP_DEFAULT_DRIFT_FRAMES, lock_permille=_capi.CMP_DEFAULT_LOCK_PERMILLE,
                    requant_millilsb2=_capi.CMP_DEFAULT_REQUANT_MILLILSB2)
    unknown = set(given) - set(_COMPARE_OPTS)
    if unknown:
        raise TypeError(f"unknown compare option(s): {sorted(unknown)}")
    o = _capi.CompareOpts(*[int(defaults[f] if given.get(f) is None else given[f]) for f in _COMPARE_OPTS])
    return o, (None if all(given.get(f) is None for f in _COMPARE_OPTS) else C.byref(o))


def compare_arena(ctx, route: int, descs, pairs, arena, blocks_per_pair=0, lag_sums=False, **opts):
    """rg_compare_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None.  `pairs`: (a, b, hint) tuples of
    indices into `descs`.  -> [CompareRecord]; with `blocks_per_pair` > 0 also a list, per pair, of its first CompareBlock rows;
    with `lag_sums` also an int64 array [pair][segment][channel (8)][2 * radius + 3].  Options (radius, segments, segment_frames,
    block_frames, drift_frames, lock_permille, requant_millilsb2, ...) None = the header's defaults."""
    L = _capi.load()
    n, n_pairs = len(descs), len(pairs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    pr = (_capi.ComparePair * max(1, n_pairs))(*[_capi.ComparePair(int(a), int(b), int(h)) for a, b, h in pairs])
    out = (_capi.CompareRecord * max(1, n_pairs))()
    o, o_p = _compare_opts(**opts)
    per = max(0, int(blocks_per_pair))
    blocks = (_capi.CompareBlock * max(1, n_pairs * per))() if per else None
    rows = np.zeros((max(1, n_pairs), max(1, min(o.segments, _capi.CMP_MAX_SEGMENTS)), _capi.CMP_MAX_CHANNELS,
                     2 * min(o.radius, _capi.CMP_MAX_RADIUS) + 3), dtype=np.int64) if lag_sums else None
    rc = L.rg_compare_arena(ctx, int(route), n, d, n_pairs, pr, o_p, arena.ctypes.data if arena.size else None, arena.size, out, blocks, per,
                            rows.ctypes.data_as(C.POINTER(C.c_int64)) if lag_sums else None)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    res = [list(out[:n_pairs])]
    if per:
        res.append([[blocks[p * per + k] for k in range(min(per, out[p].blocks))] for p in range(n_pairs)])
    if lag_sums:
        res.append(rows[:n_pairs])
    return res[0] if len(res) == 1 else tuple(res)


def compare_kernel_shape(fmt_a: int, fmt_b: int = None):
    """rg_compare_kernel_shape of a pair's two rg_sample_formats -> (piece_frames, tile_frames, strip_frames, lag_group, lds_bytes)."""
    v = [C.c_uint32() for _ in range(5)]
    rc = _capi.load().rg_compare_kernel_shape(int(fmt_a), int(fmt_a if fmt_b is None else fmt_b), *[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, f"rg_compare_kernel_shape: formats {fmt_a}, {fmt_b}")
    return tuple(x.value for x in v)


_COMPARE_FLOATS = ("lock", "gain_db", "null_unity_db", "null_db", "residual_lsb2", "worst_block_db", "gain_min_db", "gain_max_db")
_COMPARE_FIELDS = tuple(f for f, _ in _capi.CompareRecord._fields_ if f not in ("status", "reserved"))


def _clock(frames, rate, millis=False):
    """m:ss (or m:ss.mmm) of a frame index."""
    if rate <= 0:
        return f"frame {frames}"
    s = frames / rate
    return f"{int(s // 60)}:{s % 60:06.3f}" if millis else f"{int(s // 60)}:{int(s % 60):02d}"


@dataclass
class Comparison:
    """One pair of a null test (rg_compare_result): how copy b relates to the reference copy a.  The definitions are a convention
    of include/mp3rgain_amd_compare.h, held to no other tool."""
    flags: int
    a: int
    b: int
    frames_a: int
    frames_b: int
    sample_rate: int
    channels: int
    format_a: int
    format_b: int
    dropped_a: int
    dropped_b: int
    block_frames: int
    radius: int
    segments: int
    locked_segments: int
    polarity: int
    max_diff: int
    hint: int
    lag: int                 # b[n + lag] lies beside a[n]
    seg_lag_min: int
    seg_lag_max: int
    overlap: int
    a_head: int
    a_tail: int
    b_head: int
    b_tail: int
    blocks: int
    differing_blocks: int
    worst_block: int
    equal: int
    first_diff: int          # frame index in a; _capi.CMP_NONE when no sample differs
    nonfinite: int
    aa: int
    bb: int
    ab: int
    lock: float
    gain_db: float
    null_unity_db: float
    null_db: float
    residual_lsb2: float
    worst_block_db: float
    gain_min_db: float
    gain_max_db: float
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    def _has(self, bit) -> bool:
        return bool(self.flags & bit)

    @property
    def complete(self) -> bool:
        return self._has(_capi.CMP_COMPLETE)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order."""
        names = (("different sample rate", _capi.CMP_RATE), ("no overlap", _capi.CMP_NO_OVERLAP), ("identical", _capi.CMP_IDENTICAL),
                 ("same master", _capi.CMP_SAME_MASTER), ("differs", _capi.CMP_DIFFERS), ("unrelated", _capi.CMP_UNRELATED),
                 ("inverted", _capi.CMP_INVERTED), ("shifted", _capi.CMP_SHIFTED), ("lengths differ", _capi.CMP_LENGTHS), ("drifts", _capi.CMP_DRIFT),
                 ("at edge", _capi.CMP_AT_EDGE), ("no coarse match", _capi.CMP_NO_COARSE), ("channels differ", _capi.CMP_CHANNELS_DIFFER),
                 ("nonfinite", _capi.CMP_NONFINITE))
        words = [n for n, bit in names if self._has(bit)]
        if self.error is None and not self.complete:
            words.append("incomplete")
        return words

    def _placement(self) -> list:
        """Where copy b's samples lie against the reference's, as phrases."""
        out = []
        if self.b_head:
            out.append(f"starts {self.b_head} samples later")
        if self.a_head:
            out.append(f"starts {self.a_head} samples earlier")
        if self.a_tail:
            out.append(f"{self.a_tail} shorter at the end")
        if self.b_tail:
            out.append(f"{self.b_tail} longer at the end")
        return out

    @property
    def reading(self) -> str:
        """One line for a person, without the file's name."""
        if self.error is not None:
            return "failed"
        if self._has(_capi.CMP_RATE):
            return "different sample rate: not compared"
        if self._has(_capi.CMP_NO_OVERLAP):
            return "no overlap at the hint: not compared"
        head = "inverted copy, " if self._has(_capi.CMP_INVERTED) else ""
        if self._has(_capi.CMP_DRIFT):  # (segments that lock at different lags dilute the lock of the whole: asked first)
            return f"{head}same recording, drifts  (lag {self.seg_lag_min} .. {self.seg_lag_max} samples over the file)"
        if self._has(_capi.CMP_UNRELATED):
            return f"not the same recording  (best correlation {self.lock:.2f})"
        place = self._placement()
        if self._has(_capi.CMP_IDENTICAL):
            return ", ".join(["identical samples"] + place) if place else "identical"
        tail = "".join(", " + p for p in place)
        if self._has(_capi.CMP_SAME_MASTER):
            return f"{head}same master  (gain {self.gain_db:+.2f} dB, residual {self.residual_lsb2:.2f} LSB^2{tail})"
        B, rate = self.block_frames, self.sample_rate
        t0 = self.a_head + self.worst_block * B
        first = f", first difference at {_clock(self.first_diff, rate, True)}" if self.first_diff != _capi.CMP_NONE else ""
        return (f"{head}same recording, differs  (null {self.null_db:.1f} dB after {self.gain_db:+.1f} dB, worst {_clock(t0, rate)}-{_clock(t0 + B, rate)} "
                f"at {self.worst_block_db:.1f} dB{first}{tail})")


def compare_from_record(r, error=None) -> Comparison:
    """A Comparison from an rg_compare_result."""
    return Comparison(*[(float if f in _COMPARE_FLOATS else int)(getattr(r, f)) for f in _COMPARE_FIELDS], error)


def _clicks_opts(block_samples, order, ratio_permille, floor, gap, max_width, max_events):
    """rg_clicks_opts, or NULL (the header's defaults) when all are None; a None field is its default."""
    if all(v is None for v in (block_samples, order, ratio_permille, floor, gap, max_width, max_events)):
        return None
    pick = lambda v, d: d if v is None else int(v)  # noqa: E731
    return C.byref(_capi.ClicksOpts(pick(block_samples, _capi.CK_DEFAULT_BLOCK), pick(order, _capi.CK_DEFAULT_ORDER),
                                    pick(ratio_permille, _capi.CK_DEFAULT_RATIO_PERMILLE), pick(floor, _capi.CK_DEFAULT_FLOOR),
                                    pick(gap, _capi.CK_DEFAULT_GAP), pick(max_width, _capi.CK_DEFAULT_MAX_WIDTH),
                                    pick(max_events, _capi.CK_DEFAULT_MAX_EVENTS)))


def _clicks_rows(n, max_events):
    """The caller's event list: a ClicksEvent array of n rows of max_events (never empty)."""
    k = _capi.CK_DEFAULT_MAX_EVENTS if max_events is None else max(0, min(int(max_events), _capi.CK_MAX_EVENTS))
    return k, (_capi.ClicksEvent * max(1, n * k))()


def clicks_arena(ctx, route: int, descs, arena, block_samples=None, order=None, ratio_permille=None, floor=None, gap=None, max_width=None,
                 max_events=None):
    """rg_clicks_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([ClicksRecord], ClicksEvent array
    of max_events records per track, row after row).  Options None = the header's defaults."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.ClicksRecord * max(1, n))()
    k, rows = _clicks_rows(n, max_events)
    rc = L.rg_clicks_arena(ctx, int(route), n, d, _clicks_opts(block_samples, order, ratio_permille, floor, gap, max_width, max_events),
                           arena.ctypes.data if arena.size else None, arena.size, out, rows)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n]), rows


def clicks_kernel_shape(block_samples: int):
    """rg_clicks_kernel_shape of one block length -> (tile_samples, tile_blocks, fold_lanes, lds_bytes)."""
    v = [C.c_uint32() for _ in range(4)]
    rc = _capi.load().rg_clicks_kernel_shape(int(block_samples), *[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, f"rg_clicks_kernel_shape: block_samples {block_samples}")
    return tuple(x.value for x in v)


@dataclass
class ClickEvent:
    """One event of a file's list (rg_clicks_event)."""
    start: int
    width: int
    channel: int
    kind: str            # "click" or "burst"
    peak_at: int
    strength_permille: int


@dataclass
class ClickChannel:
    """One channel of a Clicks record (rg_clicks_channel)."""
    flagged: int
    clicks: int
    bursts: int
    widest: int
    first_click: int          # == frames when there is none
    strongest_at: int         # == frames when there is none
    strongest_permille: int
    fallback_blocks: int
    median_max: int


@dataclass
class Clicks:
    """One file of Analyzer.clicks (rg_clicks_result and its row of the event list): clicks and bursts per channel.  The
    definitions are a convention of include/mp3rgain_amd_clicks.h, tried on synthetic material only and held to no other tool."""
    frames: int
    sample_rate: int
    channels: int
    format: int
    dropped_frames: int
    flags: int
    block_samples: int
    order: int
    ratio_permille: int
    floor: int
    gap: int
    max_width: int
    max_events: int
    listed: int
    nonfinite: int
    events_total: int
    ch: list = field(default_factory=list)       # [ClickChannel], one per channel
    events: list = field(default_factory=list)   # [ClickEvent], the file's first `listed` events by (start, channel)
    error: Optional["ReplayGainError"] = None    # why there are no numbers; every other field is then zero

    def _has(self, bit) -> bool:
        return bool(self.flags & bit)

    @property
    def complete(self) -> bool:
        return self._has(_capi.CK_COMPLETE)

    @property
    def truncated(self) -> bool:
        return self._has(_capi.CK_TRUNCATED)

    @property
    def clicks(self) -> int:
        return sum(c.clicks for c in self.ch)

    @property
    def bursts(self) -> int:
        return sum(c.bursts for c in self.ch)

    @property
    def first_click(self):
        """(sample, channel) of the earliest click of any channel, or None."""
        have = [(c.first_click, i) for i, c in enumerate(self.ch) if c.clicks]
        return min(have) if have else None

    @property
    def strongest_click(self):
        """(strength_permille, sample, channel) of the strongest click of any channel (the earliest on a tie), or None."""
        have = [(-c.strongest_permille, c.strongest_at, i) for i, c in enumerate(self.ch) if c.clicks]
        if not have:
            return None
        s, at, i = min(have)
        return -s, at, i


def clicks_from_record(r, events=(), error=None) -> Clicks:
    """A Clicks from an rg_clicks_result and its row of rg_clicks_event."""
    names = ("flagged", "clicks", "bursts", "widest", "first_click", "strongest_at", "strongest_permille", "fallback_blocks", "median_max")
    ch = [ClickChannel(*[int(getattr(r.ch[c], f)) for f in names]) for c in range(min(int(r.channels), _capi.CK_MAX_CHANNELS))]
    evs = [ClickEvent(int(e.start), int(e.width), int(e.channel), "click" if e.kind == _capi.CK_KIND_CLICK else "burst", int(e.peak_at),
                      int(e.strength_permille)) for e in list(events)[:int(r.listed)]]
    return Clicks(int(r.frames), int(r.sample_rate), int(r.channels), int(r.format), int(r.dropped_frames), int(r.flags), int(r.block_samples),
                  int(r.order), int(r.ratio_permille), int(r.floor), int(r.gap), int(r.max_width), int(r.max_events), int(r.listed), int(r.nonfinite),
                  int(r.events), ch, evs, error)


def _fingerprint_opts(block, probes, radius, max_ber_permille):
    """rg_fingerprint_opts, or NULL (the header's defaults) when all are None; a None field is its default."""
    if block is None and probes is None and radius is None and max_ber_permille is None:
        return None
    return C.byref(_capi.FingerprintOpts(int(block or 0), int(probes or 0), int(radius or 0), int(max_ber_permille or 0)))


def fingerprint_edges(sample_rate: int):
    """rg_fingerprint_edges -> (the 34 band edges as a list, whether the rate is supported)."""
    e = (C.c_uint32 * (_capi.FP_BANDS + 1))()
    rc = _capi.load().rg_fingerprint_edges(int(sample_rate), e)
    if rc not in (0, _capi.RG_ERR_UNSUPPORTED_RATE):
        raise ReplayGainError(rc, f"rg_fingerprint_edges: rate {sample_rate}")
    return list(e), rc == 0


def fingerprint_codes(frames: int) -> int:
    """K of a track of `frames` PCM frames at a supported rate."""
    return max(0, (int(frames) - _capi.FP_FRAME) // _capi.FP_HOP) if frames >= _capi.FP_FRAME else 0


def fingerprint_arena(ctx, route: int, descs, arena, bands=True):
    """rg_fingerprint_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None ->
    ([FingerprintRecord], codes, bands): codes a uint32 array of every track's codes in track order (record.codes_at,
    record.codes), bands a float32 array [sum of F][33] (record.frames_at, record.fp_frames; None when `bands` is false)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.FingerprintRecord * max(1, n))()
    most = sum(fingerprint_codes(int(t.frames)) + 1 for t in descs)  # the frames of every track at a supported rate
    codes = np.zeros(max(1, most), dtype=np.uint32)
    e = np.zeros((max(1, most), _capi.FP_BANDS), dtype=np.float32) if bands else None
    rc = L.rg_fingerprint_arena(ctx, int(route), n, d, arena.ctypes.data if arena.size else None, arena.size, out,
                                codes.ctypes.data_as(C.POINTER(C.c_uint32)), e.ctypes.data_as(C.POINTER(C.c_float)) if bands else None)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    recs = list(out[:n])
    return recs, codes[:sum(int(r.codes) for r in recs)], (e[:sum(int(r.fp_frames) for r in recs)] if bands else None)


def fingerprint_match_codes(ctx, route: int, codes, rates, block=None, probes=None, radius=None, max_ber_permille=None):
    """rg_fingerprint_match_codes on constructed codes: `codes` a list of uint32 arrays, one per track, `rates` their sample
    rates; route 0 is the host (ctx = None), route 1 the kernel -> a structured array of the n (n - 1) / 2 pair records in
    (i, j) order, fields errors, bits, lag, flags."""
    L = _capi.load()
    n = len(codes)
    counts = np.array([len(c) for c in codes], dtype=np.uint32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in codes]) if n else np.zeros(0, dtype=np.uint32))
    r = np.array(list(rates), dtype=np.uint32)
    dt = np.dtype([("errors", "<u4"), ("bits", "<u4"), ("lag", "<i4"), ("flags", "<u4")])
    out = np.zeros(max(1, n * (n - 1) // 2), dtype=dt)
    u32p = C.POINTER(C.c_uint32)
    rc = L.rg_fingerprint_match_codes(ctx, int(route), n, counts.ctypes.data_as(u32p), r.ctypes.data_as(u32p),
                                      flat.ctypes.data_as(u32p) if flat.size else None, _fingerprint_opts(block, probes, radius, max_ber_permille),
                                      out.ctypes.data_as(C.POINTER(_capi.FingerprintPairRecord)))
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return out[:n * (n - 1) // 2]


def fingerprint_groups(n: int, pair_records):
    """rg_fingerprint_groups on the pair records of fingerprint_match_codes -> (groups, matches, number of matching pairs)."""
    L = _capi.load()
    rec = np.ascontiguousarray(pair_records)
    g, m = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    found = L.rg_fingerprint_groups(n, rec.ctypes.data_as(C.POINTER(_capi.FingerprintPairRecord)) if rec.size else None, g.ctypes.data_as(u32p),
                                    m.ctypes.data_as(u32p))
    return g[:n], m[:n], int(found)


def fingerprint_kernel_shape():
    """rg_fingerprint_kernel_shape -> (tile_codes, lanes, lds_bytes, match_lanes, lags_per_lane)."""
    v = [C.c_uint32() for _ in range(5)]
    rc = _capi.load().rg_fingerprint_kernel_shape(*[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, "rg_fingerprint_kernel_shape")
    return tuple(x.value for x in v)


@dataclass
class Fingerprint:
    """One file of Analyzer.same_recording (rg_fingerprint_result).  The fingerprint and the threshold are conventions of
    include/mp3rgain_amd_fingerprint.h, measured on this project's own synthetic material only."""
    frames: int
    sample_rate: int
    channels: int
    format: int
    dropped_frames: int
    flags: int
    fp_frames: int
    codes: int
    nonfinite_frames: int
    group: int               # the smallest index of the files this one is the same recording as (its own when alone)
    matches: int
    error: Optional["ReplayGainError"] = None  # why there is no fingerprint; every other field is then zero

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.FP_COMPLETE)

    @property
    def short(self) -> bool:
        return bool(self.flags & _capi.FP_SHORT)

    @property
    def unsupported_rate(self) -> bool:
        return bool(self.flags & _capi.FP_RATE)

    @property
    def nonfinite(self) -> bool:
        return bool(self.flags & _capi.FP_NONFINITE)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        names = (("rate", self.unsupported_rate), ("short", self.short and not self.unsupported_rate), ("nonfinite", self.nonfinite),
                 ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]


@dataclass
class SamePair:
    """One matching pair of Analyzer.same_recording (rg_fingerprint_pair): files i < j; `lag` codes of 512 samples of the
    longer file against the shorter (`probe_j`: the shorter is j)."""
    i: int
    j: int
    errors: int
    bits: int
    lag: int
    flags: int

    @property
    def ber(self) -> float:
        return self.errors / self.bits if self.bits else 0.0

    @property
    def probe_j(self) -> bool:
        return bool(self.flags & _capi.FP_PAIR_PROBE_J)

    @property
    def lag_of_j(self) -> int:
        """How many codes later than in file i the common audio lies in file j."""
        return -self.lag if self.probe_j else self.lag


def fingerprint_from_record(r, error=None) -> Fingerprint:
    """A Fingerprint from an rg_fingerprint_result."""
    return Fingerprint(int(r.frames), int(r.sample_rate), int(r.channels), int(r.format), int(r.dropped_frames), int(r.flags), int(r.fp_frames),
                       int(r.codes), int(r.nonfinite_frames), int(r.group), int(r.matches), error)


def resample_plan(sample_rate: int):
    """rg_resample_plan -> (L, M, P, whether the rate is supported)."""
    v = [C.c_uint32() for _ in range(3)]
    rc = _capi.load().rg_resample_plan(int(sample_rate), *[C.byref(x) for x in v])
    if rc not in (0, _capi.RG_ERR_UNSUPPORTED_RATE):
        raise ReplayGainError(rc, f"rg_resample_plan: rate {sample_rate}")
    return v[0].value, v[1].value, v[2].value, rc == 0


def resample_filter(up: int, down: int):
    """rg_resample_filter -> the tap table of (L, M) as a float32 array [L][P]."""
    half = 8 * max(int(up), int(down))
    taps = 1 if (up == 1 and down == 1) or up < 1 else 2 * half // int(up) + 1
    h = np.zeros((max(1, int(up)), taps), dtype=np.float32)
    rc = _capi.load().rg_resample_filter(int(up), int(down), h.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ReplayGainError(rc, f"rg_resample_filter: ({up}, {down})")
    return h


def resample_window(sample_rate: int, j: int):
    """rg_resample_window -> (b_j, p_j)."""
    b, p = C.c_uint64(), C.c_uint32()
    rc = _capi.load().rg_resample_window(int(sample_rate), int(j), C.byref(b), C.byref(p))
    if rc != 0:
        raise ReplayGainError(rc, f"rg_resample_window: rate {sample_rate}, output {j}")
    return b.value, p.value


def resample_count(sample_rate: int, frames: int) -> int:
    """M_out of a track of `frames` PCM frames (0 at an unsupported rate), in Python integers."""
    up, down, taps, ok = resample_plan(sample_rate)
    return (int(frames) - taps) * up // down + 1 if ok and frames >= taps else 0


def resample_arena(ctx, route: int, descs, arena):
    """rg_resample_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([ResampleRecord], y): y a
    float32 array of every track's resampled signal in track order (record.y_at, record.resampled)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.ResampleRecord * max(1, n))()
    y = np.zeros(max(1, sum(resample_count(int(t.sample_rate), int(t.frames)) for t in descs if t.sample_rate)), dtype=np.float32)
    rc = L.rg_resample_arena(ctx, int(route), n, d, arena.ctypes.data if arena.size else None, arena.size, out, y.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    recs = list(out[:n])
    return recs, y[:sum(int(r.resampled) for r in recs)]


def xrate_fingerprint_arena(ctx, route: int, descs, arena, bands=True):
    """rg_xrate_fingerprint_arena without an Analyzer -> ([XrateRecord], codes, bands, y), as fingerprint_arena gives them for
    the tracks' signals at 11025 Hz, and y as resample_arena's."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.XrateRecord * max(1, n))()
    counts = [resample_count(int(t.sample_rate), int(t.frames)) if t.sample_rate else 0 for t in descs]
    y = np.zeros(max(1, sum(counts)), dtype=np.float32)
    most = sum(fingerprint_codes(m) + 1 for m in counts)
    codes = np.zeros(max(1, most), dtype=np.uint32)
    e = np.zeros((max(1, most), _capi.FP_BANDS), dtype=np.float32) if bands else None
    rc = L.rg_xrate_fingerprint_arena(ctx, int(route), n, d, arena.ctypes.data if arena.size else None, arena.size, out,
                                      codes.ctypes.data_as(C.POINTER(C.c_uint32)), e.ctypes.data_as(C.POINTER(C.c_float)) if bands else None,
                                      y.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    recs = list(out[:n])
    return (recs, codes[:sum(int(r.codes) for r in recs)], (e[:sum(int(r.fp_frames) for r in recs)] if bands else None),
            y[:sum(int(r.resampled) for r in recs)])


def resample_kernel_shape():
    """rg_resample_kernel_shape -> (outputs, lanes, max_span)."""
    v = [C.c_uint32() for _ in range(3)]
    rc = _capi.load().rg_resample_kernel_shape(*[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, "rg_resample_kernel_shape")
    return tuple(x.value for x in v)


def _tempo_opts(window, hop, min_bpm):
    """rg_tempo_opts, or NULL (the header's defaults) when all are None; a None field is its default."""
    if window is None and hop is None and min_bpm is None:
        return None
    return C.byref(_capi.TempoOpts(int(window or 0), int(hop or 0), int(min_bpm or 0)))


def tempo_bands(sample_rate: int):
    """rg_tempo_bands -> (the 33 band edges as a list, whether the rate is supported)."""
    e = (C.c_uint32 * (_capi.TEMPO_BANDS + 1))()
    rc = _capi.load().rg_tempo_bands(int(sample_rate), e)
    if rc not in (0, _capi.RG_ERR_UNSUPPORTED_RATE):
        raise ReplayGainError(rc, f"rg_tempo_bands: rate {sample_rate}")
    return list(e), rc == 0


def tempo_arena(ctx, route: int, descs, arena, window=None, hop=None, min_bpm=None, bands=True):
    """rg_tempo_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([TempoRecord], onsets, bands):
    onsets a uint16 array of every track's curve in track order (record.onsets_at, record.onsets), bands a float32 array
    [sum of F][32] in track order (record.band_frames rows each; None when `bands` is false)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.TempoRecord * max(1, n))()
    most = sum(fingerprint_codes(int(t.frames)) + 1 for t in descs)  # the frames of every track at a supported rate
    onsets = np.zeros(max(1, most), dtype=np.uint16)
    e = np.zeros((max(1, most), _capi.TEMPO_BANDS), dtype=np.float32) if bands else None
    rc = L.rg_tempo_arena(ctx, int(route), n, d, arena.ctypes.data if arena.size else None, arena.size, _tempo_opts(window, hop, min_bpm), out,
                          onsets.ctypes.data_as(C.POINTER(C.c_uint16)), e.ctypes.data_as(C.POINTER(C.c_float)) if bands else None)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    recs = list(out[:n])
    return recs, onsets[:sum(int(r.onsets) for r in recs)], (e[:sum(int(r.band_frames) for r in recs)] if bands else None)


def tempo_from_onsets(ctx, route: int, onsets, rates, window=None, hop=None, min_bpm=None):
    """rg_tempo_from_onsets on constructed curves: `onsets` a list of uint16 arrays, one per track, `rates` their sample rates;
    route 0 is the host (ctx = None), route 1 the kernels -> ([TempoRecord], acf): acf an int64 array [n][W], C of every track."""
    L = _capi.load()
    n = len(onsets)
    counts = np.array([len(o) for o in onsets], dtype=np.uint32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.uint16) for o in onsets]) if n else np.zeros(0, dtype=np.uint16))
    r = np.array(list(rates), dtype=np.uint32)
    W = int(window or _capi.TEMPO_WINDOW)
    out = (_capi.TempoRecord * max(1, n))()
    acf = np.zeros((max(1, n), max(1, min(W, _capi.TEMPO_MAX_WINDOW))), dtype=np.int64)
    u32p = C.POINTER(C.c_uint32)
    rc = L.rg_tempo_from_onsets(ctx, int(route), n, counts.ctypes.data_as(u32p), r.ctypes.data_as(u32p),
                                flat.ctypes.data_as(C.POINTER(C.c_uint16)) if flat.size else None, _tempo_opts(window, hop, min_bpm), out,
                                acf.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n]), acf[:n]


def tempo_kernel_shape():
    """rg_tempo_kernel_shape -> (tile_onsets, lanes, lds_bytes, acf_lanes, lags_per_lane)."""
    v = [C.c_uint32() for _ in range(5)]
    rc = _capi.load().rg_tempo_kernel_shape(*[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, "rg_tempo_kernel_shape")
    return tuple(x.value for x in v)


@dataclass
class Tempo:
    """One file of Analyzer.tempo (rg_tempo_result).  The estimator is a convention of include/mp3rgain_amd_tempo.h, tried on
    this project's own synthetic material only; the reading lies in [min_bpm, 2 min_bpm) by convention."""
    frames: int
    sample_rate: int
    channels: int
    format: int
    dropped_frames: int
    flags: int
    onsets: int
    windows: int
    period16: int
    harmonics: int
    bpm_milli: int
    confidence_permille: int
    stable_permille: int
    first_beat: int
    nonfinite_frames: int
    error: Optional["ReplayGainError"] = None  # why there is no reading; every other field is then zero

    @property
    def found(self) -> bool:
        return self.error is None and self.period16 != 0

    @property
    def bpm(self) -> Optional[float]:
        return self.bpm_milli / 1000.0 if self.found else None

    @property
    def confidence(self) -> float:
        return self.confidence_permille / 1000.0

    @property
    def steady(self) -> float:
        return self.stable_permille / 1000.0

    @property
    def first_beat_seconds(self) -> Optional[float]:
        return self.first_beat / self.sample_rate if self.found and self.sample_rate else None

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.TEMPO_COMPLETE)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        f = self.flags
        names = (("rate", f & _capi.TEMPO_RATE), ("short", f & _capi.TEMPO_SHORT and not f & _capi.TEMPO_RATE), ("range", f & _capi.TEMPO_RANGE),
                 ("none", f & _capi.TEMPO_NONE), ("nonfinite", f & _capi.TEMPO_NONFINITE), ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]


def tempo_from_record(r, error=None) -> Tempo:
    """A Tempo from an rg_tempo_result."""
    return Tempo(int(r.frames), int(r.sample_rate), int(r.channels), int(r.format), int(r.dropped_frames), int(r.flags), int(r.onsets), int(r.windows),
                 int(r.period16), int(r.harmonics), int(r.bpm_milli), int(r.confidence_permille), int(r.stable_permille), int(r.first_beat),
                 int(r.nonfinite_frames), error)


def _key_opts(segment):
    """rg_key_opts, or NULL (the header's default) when `segment` is None."""
    return None if segment is None else C.byref(_capi.KeyOpts(int(segment)))


def key_bands(sample_rate: int):
    """rg_key_bands -> (D, the 61 band edges as a list (None at an unsupported rate), whether the rate is supported)."""
    e = (C.c_uint32 * (_capi.KEY_BANDS + 1))()
    d = C.c_uint32()
    rc = _capi.load().rg_key_bands(int(sample_rate), C.byref(d), e)
    if rc not in (0, _capi.RG_ERR_UNSUPPORTED_RATE):
        raise ReplayGainError(rc, f"rg_key_bands: rate {sample_rate}")
    return d.value, (list(e) if rc == 0 else None), rc == 0


def key_filter(decim: int):
    """rg_key_filter -> the 16 D + 1 taps of factor D as a float32 array."""
    taps = np.zeros(_capi.KEY_TAPS_PER_DECIM * int(decim) + 1, dtype=np.float32)
    rc = _capi.load().rg_key_filter(int(decim), taps.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ReplayGainError(rc, f"rg_key_filter: factor {decim}")
    return taps


def key_arena(ctx, route: int, descs, arena, segment=None, bands=True):
    """rg_key_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([KeyRecord], y, bands, chroma): y a
    float32 array of every track's decimated signal in track order (record.decimated each), bands a float32 array [sum of F][60]
    (None when `bands` is false), chroma a uint16 array [sum of F][12] (record.chroma_at, record.rows)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.KeyRecord * max(1, n))()
    most_y = sum(int(t.frames) for t in descs)
    most_rows = sum(int(t.frames) // _capi.KEY_HOP + 1 for t in descs)
    y = np.zeros(max(1, most_y), dtype=np.float32)
    e = np.zeros((max(1, most_rows), _capi.KEY_BANDS), dtype=np.float32) if bands else None
    chroma = np.zeros((max(1, most_rows), _capi.KEY_CHROMA), dtype=np.uint16)
    rc = L.rg_key_arena(ctx, int(route), n, d, arena.ctypes.data if arena.size else None, arena.size, _key_opts(segment), out,
                        y.ctypes.data_as(C.POINTER(C.c_float)), e.ctypes.data_as(C.POINTER(C.c_float)) if bands else None,
                        chroma.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    recs = list(out[:n])
    rows = sum(int(r.rows) for r in recs)
    return recs, y[:sum(int(r.decimated) for r in recs)], (e[:rows] if bands else None), chroma[:rows]


def key_from_chroma(ctx, route: int, chroma, segment=None):
    """rg_key_from_chroma on constructed rows: `chroma` a list of uint16 arrays [F][12], one per track; route 0 is the host
    (ctx = None), route 1 the finish kernel -> [KeyRecord]."""
    L = _capi.load()
    n = len(chroma)
    rows = [np.asarray(c, dtype=np.uint16).reshape(-1, _capi.KEY_CHROMA) for c in chroma]
    counts = np.array([len(c) for c in rows], dtype=np.uint32)
    flat = np.ascontiguousarray(np.concatenate(rows) if n else np.zeros((0, _capi.KEY_CHROMA), dtype=np.uint16))
    out = (_capi.KeyRecord * max(1, n))()
    rc = L.rg_key_from_chroma(ctx, int(route), n, counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                              flat.ctypes.data_as(C.POINTER(C.c_uint16)) if flat.size else None, _key_opts(segment), out)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n])


def key_kernel_shape():
    """rg_key_kernel_shape -> (decim_outputs, decim_lanes, tile_rows, tile_lanes, tile_lds_bytes)."""
    v = [C.c_uint32() for _ in range(5)]
    rc = _capi.load().rg_key_kernel_shape(*[C.byref(x) for x in v])
    if rc != 0:
        raise ReplayGainError(rc, "rg_key_kernel_shape")
    return tuple(x.value for x in v)


KEY_TONICS = ("C", "C#", "D", "Eb", "E", "F", "F#", "G", "Ab", "A", "Bb", "B")


def key_name(key: int) -> str:
    """`A minor` for key 12 mode + tonic."""
    return f"{KEY_TONICS[key % 12]} {'minor' if key // 12 else 'major'}"


def key_camelot(key: int) -> str:
    """The Camelot wheel: C major is 8B, A minor 8A; a minor key has the number of its relative major."""
    tonic, minor = key % 12, key // 12
    if minor:
        tonic = (tonic + 3) % 12
    return f"{((7 * tonic) % 12 + 7) % 12 + 1}{'A' if minor else 'B'}"


def key_open_key(key: int) -> str:
    """Open Key notation: Camelot number n -> ((n + 4) mod 12) + 1, `d` for major and `m` for minor; 8B is 1d."""
    cam = key_camelot(key)
    return f"{(int(cam[:-1]) + 4) % 12 + 1}{'m' if key // 12 else 'd'}"


@dataclass
class Key:
    """One file of Analyzer.key (rg_key_result).  The estimator is a convention of include/mp3rgain_amd_key.h, tried on this
    project's own synthetic material only."""
    frames: int
    sample_rate: int
    channels: int
    format: int
    dropped_frames: int
    flags: int
    decim: int
    decimated: int
    rows: int
    silent_rows: int
    nonfinite_frames: int
    key: int
    tonic: int
    mode: int
    correlation_permille: int
    margin_permille: int
    segments: int
    stable_permille: int
    error: Optional["ReplayGainError"] = None  # why there is no reading; every other field is then zero

    @property
    def found(self) -> bool:
        return self.error is None and not self.flags & (_capi.KEY_SHORT | _capi.KEY_RATE | _capi.KEY_NONE)

    @property
    def name(self) -> Optional[str]:
        return key_name(self.key) if self.found else None

    @property
    def camelot(self) -> Optional[str]:
        return key_camelot(self.key) if self.found else None

    @property
    def open_key(self) -> Optional[str]:
        return key_open_key(self.key) if self.found else None

    @property
    def correlation(self) -> float:
        return self.correlation_permille / 1000.0

    @property
    def margin(self) -> float:
        return self.margin_permille / 1000.0

    @property
    def steady(self) -> float:
        return self.stable_permille / 1000.0

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.KEY_COMPLETE)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        f = self.flags
        names = (("rate", f & _capi.KEY_RATE), ("short", f & _capi.KEY_SHORT and not f & _capi.KEY_RATE), ("none", f & _capi.KEY_NONE),
                 ("nonfinite", f & _capi.KEY_NONFINITE), ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]


def key_from_record(r, error=None) -> Key:
    """A Key from an rg_key_result."""
    return Key(int(r.frames), int(r.sample_rate), int(r.channels), int(r.format), int(r.dropped_frames), int(r.flags), int(r.decim), int(r.decimated),
               int(r.rows), int(r.silent_rows), int(r.nonfinite_frames), int(r.key), int(r.tonic), int(r.mode), int(r.correlation_permille),
               int(r.margin_permille), int(r.segments), int(r.stable_permille), error)


def _ancestry_opts(segments, granules, z_min, iso_min, active_floor):
    """rg_ancestry_opts, or NULL (the header's defaults) when all are None.  segments = 0 is the whole plane as one segment."""
    if segments is None and granules is None and z_min is None and iso_min is None and active_floor is None:
        return None
    return C.byref(_capi.AncestryOpts(_capi.ANC_SEGMENTS if segments is None else int(segments),
                                      _capi.ANC_GRANULES if granules is None else int(granules),
                                      0.0 if z_min is None else float(z_min), 0.0 if iso_min is None else float(iso_min),
                                      0.0 if active_floor is None else float(active_floor), 0))


def ancestry_arena(ctx, route: int, descs, arena, segments=None, granules=None, z_min=None, iso_min=None, active_floor=None, counts=True):
    """rg_ancestry_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([AncestryRecord], counts),
    counts a uint64 array [track][view][0 = small, 1 = active][576] (None when `counts` is false)."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.AncestryRecord * max(1, n))()
    cnt = np.zeros((max(1, n), _capi.ANC_MAX_VIEWS, 2, _capi.ANC_ALIGNMENTS), dtype=np.uint64) if counts else None
    rc = L.rg_ancestry_arena(ctx, int(route), n, d, _ancestry_opts(segments, granules, z_min, iso_min, active_floor),
                             arena.ctypes.data if arena.size else None, arena.size, out,
                             cnt.ctypes.data_as(C.POINTER(C.c_uint64)) if counts else None)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n]), (cnt[:n] if counts else None)


def ancestry_kernel_shape():
    """rg_ancestry_kernel_shape -> (phases, tile_granules, lanes, lds_bytes)."""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = _capi.load().rg_ancestry_kernel_shape(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    if rc != 0:
        raise ReplayGainError(rc, "rg_ancestry_kernel_shape")
    return a.value, b.value, c.value, d.value


@dataclass
class AncestryView:
    """One view of an Ancestry (rg_ancestry_view, include/mp3rgain_amd_ancestry.h)."""
    kind: int                # the channel's index, 8 = mid, 9 = side
    offset: int              # r*: the alignment with the largest share of small lines
    ratio: float             # small / active there
    second: float            # the next-best ratio
    p0: float                # the pooled ratio of all other alignments
    z: float
    iso: float               # ratio / second
    small: int
    active: int
    active_total: int
    flagged: bool
    nonfinite: int

    @property
    def name(self) -> str:
        return {_capi.ANC_VIEW_MID: "mid", _capi.ANC_VIEW_SIDE: "side"}.get(self.kind, f"ch{self.kind}")


@dataclass
class Ancestry:
    """One file of Analyzer.ancestry (rg_ancestry_result).  The verdict is a convention of include/mp3rgain_amd_ancestry.h,
    tried on this project's own encoder only and held to no other ancestry checker; "no grid found" proves nothing."""
    frames: int
    sample_rate: int
    format: int
    dropped_frames: int
    flags: int
    segments: int
    granules: int
    grid_offset: int
    best_view: Optional[int]
    z: float
    iso: float
    views: list              # [AncestryView]
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.ANC_COMPLETE)

    @property
    def mp3_grid(self) -> bool:
        return bool(self.flags & _capi.ANC_MP3_GRID)

    @property
    def midside(self) -> bool:
        return bool(self.flags & _capi.ANC_MIDSIDE)

    @property
    def nonfinite(self) -> bool:
        return bool(self.flags & _capi.ANC_NONFINITE)

    @property
    def short(self) -> bool:
        return bool(self.flags & _capi.ANC_SHORT)

    @property
    def silent(self) -> bool:
        return bool(self.flags & _capi.ANC_SILENT)

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        names = (("mp3-grid", self.mp3_grid), ("mid/side", self.midside), ("silent", self.silent), ("short", self.short),
                 ("nonfinite", self.nonfinite), ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]

    @property
    def summary(self) -> str:
        """`mp3 grid at +R (z 30.1, x2.35, mid/side)` or `no grid found`."""
        if not self.mp3_grid:
            return "no grid found"
        return f"mp3 grid at +{self.grid_offset} (z {self.z:.1f}, x{self.iso:.2f}{', mid/side' if self.midside else ''})"


def ancestry_from_record(r, error=None) -> Ancestry:
    """An Ancestry from an rg_ancestry_result."""
    views = []
    for k in range(int(r.views)):
        v = r.view[k]
        views.append(AncestryView(int(v.kind), int(v.offset), float(v.ratio), float(v.second), float(v.p0), float(v.z), float(v.iso),
                                  int(v.small), int(v.active), int(v.active_total), bool(v.flagged), int(v.nonfinite)))
    best = None if int(r.best_view) == _capi.ANC_NO_VIEW or error is not None else int(r.best_view)
    return Ancestry(int(r.frames), int(r.sample_rate), int(r.format), int(r.dropped_frames), int(r.flags), int(r.segments), int(r.granules),
                    int(r.grid_offset), best, float(r.z), float(r.iso), views, error)


def _spectrum_opts(edge_db, min_cutoff_hz):
    """rg_spectrum_opts, or NULL (the header's defaults) when both are None."""
    if edge_db is None and min_cutoff_hz is None:
        return None
    return C.byref(_capi.SpectrumOpts(_capi.SPEC_EDGE_DB if edge_db is None else float(edge_db),
                                      _capi.SPEC_MIN_CUTOFF_HZ if min_cutoff_hz is None else float(min_cutoff_hz)))


def _spectrum_bands(n):
    return np.zeros((max(1, n), _capi.SPEC_MAX_CHANNELS, _capi.SPEC_BANDS), dtype=np.float64)


def spectrum_arena(ctx, route: int, descs, arena, edge_db=None, min_cutoff_hz=None, bands=True):
    """rg_spectrum_arena without an Analyzer: routes 0 and 2 are host code and take ctx = None -> ([SpectrumRecord], E) with E
    a float64 array [track, 8, 256] of band energies (None when `bands` is false).  Both options None = the header's defaults."""
    L = _capi.load()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    out = (_capi.SpectrumRecord * max(1, n))()
    e = _spectrum_bands(n) if bands else None
    rc = L.rg_spectrum_arena(ctx, int(route), n, d, _spectrum_opts(edge_db, min_cutoff_hz), arena.ctypes.data if arena.size else None, arena.size, out,
                             e.ctypes.data_as(C.POINTER(C.c_double)) if bands else None)
    if rc != 0:
        raise ReplayGainError(rc, L.rg_last_error(ctx).decode("utf-8", "replace"))
    return list(out[:n]), (e[:n] if bands else None)


def spectrum_kernel_shape():
    """rg_spectrum_kernel_shape -> (frame, hop, bands, frames_per_tile)."""
    f, h, b, t = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _capi.load().rg_spectrum_kernel_shape(C.byref(f), C.byref(h), C.byref(b), C.byref(t))
    return f.value, h.value, b.value, t.value


def spectrum_verdict(p, analysed_frames: int, sample_rate: int, edge_db=None, min_cutoff_hz=None):
    """rg_spectrum_verdict on 256 band levels -> SpectrumChannel (the C record)."""
    L = _capi.load()
    a = np.ascontiguousarray(p, dtype=np.float64)
    if a.shape != (_capi.SPEC_BANDS,):
        raise ValueError("spectrum_verdict takes 256 numbers")
    out = _capi.SpectrumChannel()
    rc = L.rg_spectrum_verdict(a.ctypes.data_as(C.POINTER(C.c_double)), int(analysed_frames), int(sample_rate), _spectrum_opts(edge_db, min_cutoff_hz),
                               C.byref(out))
    if rc != 0:
        raise ReplayGainError(rc, "rg_spectrum_verdict: a sample rate of 0, or an option that is not greater than 0")
    return out


@dataclass
class ChannelSpectrum:
    """One channel of a Spectrum (rg_spectrum_channel, include/mp3rgain_amd_spectrum.h)."""
    cutoff_hz: float         # the upper edge of the last band in front of the edge; sample_rate / 2 when there is no edge
    edge_db: float           # the 8 bands below the edge over the 8 above it; 0 when there is no edge
    analysed_frames: int
    skipped_frames: int      # frames of a float plane with a NaN or Inf
    flags: int
    bands: Optional[object] = None  # E[j]: 256 float64, when they were asked for

    @property
    def bandlimited(self) -> bool:
        return bool(self.flags & _capi.SPEC_BANDLIMITED)

    @property
    def upsampled(self) -> bool:
        return bool(self.flags & _capi.SPEC_UPSAMPLED)

    @property
    def levels_db(self):
        """The 256 band levels in dB relative to the loudest band (None without bands; -inf for an empty band)."""
        if self.bands is None:
            return None
        e = np.asarray(self.bands, dtype=np.float64)
        top = float(e.max()) if e.size else 0.0
        if not top > 0.0:
            return [float("-inf")] * len(e)
        with np.errstate(divide="ignore"):
            return [float(x) for x in 10.0 * np.log10(e / top)]


@dataclass
class Spectrum:
    """One file of Analyzer.spectrum (rg_spectrum_result): where the spectrum ends."""
    frames: int
    sample_rate: int
    format: int              # rg_sample_format of the planes that were transformed
    dropped_frames: int
    cutoff_hz: float         # the maximum over the channels
    flags: int
    channels: list           # [ChannelSpectrum]
    error: Optional["ReplayGainError"] = None  # why there are no numbers; every other field is then zero

    @property
    def bandlimited(self) -> bool:
        return bool(self.flags & _capi.SPEC_BANDLIMITED)

    @property
    def upsampled(self) -> bool:
        return bool(self.flags & _capi.SPEC_UPSAMPLED)

    @property
    def short(self) -> bool:
        return bool(self.flags & _capi.SPEC_SHORT)

    @property
    def nonfinite(self) -> bool:
        return bool(self.flags & _capi.SPEC_NONFINITE)

    @property
    def complete(self) -> bool:
        return bool(self.flags & _capi.SPEC_COMPLETE)

    @property
    def cut_channels(self) -> list:
        """The indices of the band-limited channels."""
        return [k for k, c in enumerate(self.channels) if c.bandlimited]

    @property
    def lowest_cut(self) -> Optional["ChannelSpectrum"]:
        """The band-limited channel with the lowest cutoff (the first of equals); None when no channel is band-limited.  The
        record's own cutoff_hz is the maximum over all channels, which is Nyquist as soon as one channel has no edge."""
        cut = [c for c in self.channels if c.bandlimited]
        return min(cut, key=lambda c: c.cutoff_hz) if cut else None

    @property
    def edge_db(self) -> float:
        """The edge of `lowest_cut`; 0 when no channel is band-limited."""
        c = self.lowest_cut
        return c.edge_db if c is not None else 0.0

    @property
    def verdicts(self) -> list:
        """The flags as words, in a fixed order; ["ok"] when there is nothing to report."""
        names = (("bandlimited", self.bandlimited), ("upsampled", self.upsampled), ("short", self.short), ("nonfinite", self.nonfinite),
                 ("incomplete", self.error is None and not self.complete))
        return [n for n, on in names if on] or ["ok"]

    @property
    def words(self) -> str:
        """One line of plain words."""
        if self.short or not any(c.analysed_frames for c in self.channels):
            return "too short to analyse"
        c, cut = self.lowest_cut, self.cut_channels
        if c is None:
            return "no cutoff below Nyquist"
        some = "" if len(cut) == len(self.channels) else f" (channel{'s' if len(cut) > 1 else ''} {', '.join(str(k) for k in cut)} of {len(self.channels)})"
        if self.upsampled:
            top = max(x.cutoff_hz for x in self.channels if x.upsampled)
            return f"{self.sample_rate / 1000:g} kHz file with nothing above {top / 1000:.1f} kHz{some}"
        return f"cut off at {c.cutoff_hz / 1000:.1f} kHz, edge {c.edge_db:.0f} dB{some}"


def spectrum_from_record(r, error=None, bands=None) -> Spectrum:
    """A Spectrum from an rg_spectrum_result (and its [8, 256] band energies)."""
    ch = []
    for k in range(int(r.channels)):
        c = r.ch[k]
        ch.append(ChannelSpectrum(float(c.cutoff_hz), float(c.edge_db), int(c.analysed_frames), int(c.skipped_frames), int(c.flags),
                                  None if bands is None else np.array(bands[k], dtype=np.float64)))
    return Spectrum(int(r.frames), int(r.sample_rate), int(r.format), int(r.dropped_frames), float(r.cutoff_hz), int(r.flags), ch, error)


@dataclass
class FlacVerifyResult:
    """One file of Analyzer.verify_flac (rg_flac_verify_result): the decoded PCM's MD5 against STREAMINFO's signature."""
    has_signature: bool      # STREAMINFO's MD5 is not all zero
    md5_match: bool          # only with has_signature: md5_decoded == md5_stream
    length_match: bool       # total_samples is 0 (unknown) or equals frames
    complete: bool           # no frame was dropped
    frames: int              # PCM frames per channel that were decoded and hashed
    total_samples: int       # STREAMINFO
    audio_frames: int
    dropped_frames: int
    md5_stream: bytes
    md5_decoded: bytes
    error: Optional["ReplayGainError"] = None  # why there is no decode; every other field is then zero

    @property
    def verified(self) -> bool:
        return self.error is None and self.has_signature and self.md5_match and self.length_match and self.complete


@dataclass
class RipChecksums:
    """One file of Analyzer.rip_checksums (rg_rip_result, include/mp3rgain_amd_rip.h): the numbers a ripper's log holds."""
    crc32: int               # CRC-32 of the PCM's interleaved bytes (EAC's "Copy CRC")
    crc32_nonnull: int       # the same with null samples left out
    arv1: int                # AccurateRip v1 / v2 signatures
    arv2: int
    frames: int              # PCM frames per channel that were hashed
    null_samples: int
    sample_rate: int
    dropped_frames: int      # FLAC frames the decode route dropped
    cd_rate: bool            # 44100 Hz
    cd_frames: bool          # frames is a whole number of CD sectors (588 frames)
    complete: bool           # no frame was dropped
    first_track: bool = False  # what the call was told about the file's place on its disc
    last_track: bool = False
    error: Optional["ReplayGainError"] = None  # why there are no checksums; every other field is then zero


@dataclass
class RipOffsetSignatures:
    """Analyzer.rip_offset_signatures (rg_rip_offset_signatures): a disc's AccurateRip signatures at every drive offset."""
    tracks: list             # [RipChecksums], what rip_checksums gives for the same files and flags
    radius: int
    arv1: np.ndarray         # uint32 [n, 2 radius + 1]: track t at offset o is [t][o + radius]
    arv2: np.ndarray

    def at(self, track: int, offset: int):
        """(arv1, arv2) of track `track` read `offset` frames later on the disc."""
        return int(self.arv1[track][offset + self.radius]), int(self.arv2[track][offset + self.radius])


@dataclass
class PcmTrack:
    """Decoded audio of one file: planar channels (float32 in [-1,1], int16 or int32)."""

    channels: Sequence[np.ndarray]
    sample_rate: int
    file_type: AudioFileType = AudioFileType.Mp3
    channel_weights: Optional[Sequence[float]] = None  # EBU R 128 only: up to 8 weights, one per channel (missing ones: 0)
    _fmt: int = field(init=False, default=0)

    def __post_init__(self):
        if len(self.channels) == 0:
            raise ValueError("No audio track found")  # src/replaygain.rs:834-836
        if self.channel_weights is not None:
            self.channel_weights = [float(w) for w in self.channel_weights]
            if len(self.channel_weights) > 8:
                raise ValueError("at most 8 channel weights")
        chans = [np.ascontiguousarray(c) for c in self.channels]
        dt = chans[0].dtype
        if dt not in _NP_FMT:
            raise TypeError(f"unsupported sample dtype {dt}")
        for c in chans:
            if c.dtype != dt or c.shape != chans[0].shape or c.ndim != 1:
                raise ValueError("channels must be 1-D arrays of one dtype and length")
        self.channels = chans
        self._fmt = _NP_FMT[dt]

    @property
    def frames(self) -> int:
        return int(self.channels[0].shape[0])


_R128_MODES = {"pair": _capi.R128_CHANNELS_PAIR, "layout": _capi.R128_CHANNELS_LAYOUT}


def _r128_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in _R128_MODES:
            raise ValueError(f"unknown R 128 channel mode {mode!r} (pair, layout)")
        return _R128_MODES[mode]
    return int(mode)


def r128_layout_weights(channels: int, mask: int = 0) -> List[float]:
    """The BS.1770 weights of a layout of 1 to 8 channels (rg_r128_layout_weights; host only): channel i is the i-th set bit
    of the WAVE channel mask `mask`, 0 = the default layout of that many channels (the FLAC channel order)."""
    w = _capi.R128ChannelWeights()
    rc = _capi.load().rg_r128_layout_weights(int(channels), int(mask), C.byref(w))
    if rc != _capi.RG_OK:
        raise ReplayGainError(rc, f"Unsupported channel count for layout analysis: {channels} (1 to 8)")
    return [float(w.w[i]) for i in range(int(channels))]


def _to_dynamics(d) -> Optional[R128Dynamics]:
    if d is None:
        return None
    return R128Dynamics(d.loudness_range_lu, d.range_low_lufs, d.range_high_lufs, d.max_momentary_lufs, d.max_short_term_lufs,
                        d.st_blocks, d.st_blocks_gated)


def _to_r128(r, file_type, dyn=None) -> R128Result:
    return R128Result(r.loudness_lufs, r.gain_db, r.sample_peak, r.true_peak, r.sample_rate, r.blocks, r.blocks_gated, r.flags,
                      AudioFileType(int(file_type)), _to_dynamics(dyn))


def _to_r128_album(tracks, a, dyn=None) -> R128AlbumResult:
    return R128AlbumResult(tracks, a.loudness_lufs, a.gain_db, a.sample_peak, a.true_peak, a.blocks, a.blocks_gated, _to_dynamics(dyn))


def _split_blocks(z, counts):
    out, p = [], 0
    for k in counts:
        out.append(z[p:p + k].copy())
        p += k
    return out


def is_available() -> bool:
    """replaygain::is_available (src/replaygain.rs:1119-1121): the library is present."""
    try:
        return bool(_capi.load().rg_is_available())
    except (ImportError, OSError):
        return False


def db_to_steps(db: float) -> int:
    return _capi.load().rg_db_to_steps(db)


def steps_to_db(steps: int) -> float:
    return _capi.load().rg_steps_to_db(steps)


def clip_limit_steps(steps: int, gain_db: float, peak: float, prevent_clipping: bool, wrap_gain: bool = False) -> int:
    """The -k rule of the CLI (src/main.rs:2033-2058)."""
    return _capi.load().rg_clip_limit_steps(steps, gain_db, peak, int(prevent_clipping), int(wrap_gain))


def pack_tracks(tracks: Sequence[PcmTrack]):
    """Lay the tracks out in one planar arena -> (uint8 arena, TrackDesc array).

    Track t, channel c lives at offset_bytes + c * frames * itemsize; each track starts on a
    16-byte boundary.  All channels are packed so that find_peak_amplitude sees every channel;
    the analysis itself reads channels 0 and 1 only (src/replaygain.rs:971).
    """
    descs = (_capi.TrackDesc * max(1, len(tracks)))()
    sizes, off = [], 0
    for t in tracks:
        nbytes = sum(c.nbytes for c in t.channels)
        sizes.append((off, nbytes))
        off = (off + nbytes + 15) & ~15
    arena = np.zeros(max(off, 16), dtype=np.uint8)
    for i, t in enumerate(tracks):
        o, _ = sizes[i]
        p = o
        for c in t.channels:
            arena[p:p + c.nbytes] = c.view(np.uint8)
            p += c.nbytes
        descs[i].offset_bytes = o
        descs[i].frames = t.frames
        descs[i].sample_rate = t.sample_rate
        descs[i].channels = len(t.channels)
        descs[i].format = t._fmt
    return arena, descs


class Analyzer:
    """One rg_ctx (one GPU).  Not thread-safe, like the single-threaded reference."""

    def __init__(self, device: int = 0):
        self._lib = _capi.load()
        self._ctx = self._lib.rg_create(device)
        if not self._ctx:
            msg = self._lib.rg_last_error(None).decode()
            raise ReplayGainError(_capi.RG_ERR_NO_DEVICE, msg)
        self.device = device

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            if not getattr(self, "_borrowed", False):  # a Node's context (Node.analyzer) dies with the node
                self._lib.rg_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != _capi.RG_OK:
            raise ReplayGainError(rc, self._lib.rg_last_error(self._ctx).decode())

    @staticmethod
    def _file_args(files, record):
        """What a per-file call takes -> (`files` as a c_char_p array, zeroed records of ctypes type `record`), one entry per
        file and never fewer than one."""
        n = max(1, len(files))
        return (C.c_char_p * n)(*[os.fsencode(os.fspath(f)) for f in files]), (record * n)()

    def _file_records(self, out, n):
        """(record, its ReplayGainError or None) for each of the `n` files of the per-file call that has just filled `out`."""
        for i in range(n):
            err = None
            if out[i].status != 0:
                err = ReplayGainError(int(out[i].status), self._lib.rg_tracks_error(self._ctx, i).decode("utf-8", "replace"))
            yield out[i], err

    @property
    def handle(self):
        return self._ctx

    def set_stream(self, hip_stream: Optional[int]):
        """Attach a HIP stream handle (0 = the default stream, e.g. torch.cuda.current_stream().cuda_stream);
        None detaches."""
        if hip_stream is None:
            self._check(self._lib.rg_set_stream(self._ctx, None, 0))
        else:
            self._check(self._lib.rg_set_stream(self._ctx, hip_stream or None, 1))

    def batch_stream(self) -> int:
        """HIP stream handle of the most recent enqueue (rg_batch_stream): issue the album collective on it."""
        return int(self._lib.rg_batch_stream(self._ctx) or 0)

    def wait_user_stream(self):
        """Order the next enqueue behind what the attached stream has been given so far."""
        self._check(self._lib.rg_wait_user_stream(self._ctx))

    def set_kernel(self, variant: int):
        self._check(self._lib.rg_set_kernel(self._ctx, variant))

    def set_tuning(self, key: int, value: int):
        """key 1: segment length of variant 2 (frames); key 2: lane target; 0 = default."""
        self._check(self._lib.rg_set_tuning(self._ctx, key, value))

    # -- synchronous, host PCM ----------------------------------------------------------------
    def analyze_tracks(self, tracks: Sequence[PcmTrack], return_histograms: bool = False):
        """`-r` mode: analyze_track for each track (src/replaygain.rs:929-941)."""
        n = len(tracks)
        arena, descs = pack_tracks(tracks)
        out = (_capi.TrackResult * max(1, n))()
        hist = np.zeros((max(1, n), _capi.HISTOGRAM_SIZE), dtype=np.uint32) if return_histograms else None
        self._check(self._lib.rg_analyze_pcm_batch(
            self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, out,
            hist.ctypes.data if hist is not None else None))
        res = [_to_result(out[i], tracks[i].file_type) for i in range(n)]
        return (res, hist[:n]) if return_histograms else res

    def analyze_track(self, track: PcmTrack) -> ReplayGainResult:
        return self.analyze_tracks([track])[0]

    def analyze_album(self, tracks: Sequence[PcmTrack], return_histogram: bool = False):
        """analyze_album (src/replaygain.rs:1033-1074) on one GPU."""
        n = len(tracks)
        arena, descs = pack_tracks(tracks)
        out = (_capi.TrackResult * max(1, n))()
        alb = _capi.AlbumResult()
        hist = np.zeros(_capi.HISTOGRAM_SIZE, dtype=np.uint32) if return_histogram else None
        self._check(self._lib.rg_analyze_album_pcm(
            self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, out, C.byref(alb),
            hist.ctypes.data if hist is not None else None))
        res = AlbumGainResult([_to_result(out[i], tracks[i].file_type) for i in range(n)],
                              alb.album_loudness_db, alb.album_gain_db, alb.album_peak)
        return (res, hist) if return_histogram else res

    # -- EBU R 128 / ReplayGain 2.0 (include/mp3rgain_amd_r128.h) ------------------------------------
    def set_tuning_r128(self, key: int, value: int):
        """key 1: hops per lane of the loudness kernel; 0 = chosen from the batch.  key 2: an album's loudness range selection,
        0 = chosen by the library, 1 = one workgroup, 2 = wide counting passes."""
        self._check(self._lib.rg_r128_set_tuning(self._ctx, key, value))

    def set_channel_mode_r128(self, mode):
        """"pair" (the default): channels 0 and 1 of every track, weight 1.0.  "layout": every track weighted by its channel
        layout (r128_layout_weights; files: by their container's channel mask)."""
        self._check(self._lib.rg_r128_set_channel_mode(self._ctx, _r128_mode(mode)))
        self._r128_layout = _r128_mode(mode) == _capi.R128_CHANNELS_LAYOUT

    def _r128_weighted(self, tracks, first, true_peak, return_blocks, dynamics, return_short_term):
        """rg_r128_analyze_pcm_weighted: tracks that carry channel_weights use them, the others the weights the context's
        channel mode gives them.  first: None (no albums) or the albums' first tracks.  -> out, alb, dyn, adyn, extra"""
        n = len(tracks)
        arena, descs = pack_tracks(tracks)
        weights = (_capi.R128ChannelWeights * max(1, n))()
        layout = getattr(self, "_r128_layout", False)
        for i, t in enumerate(tracks):
            cw = t.channel_weights
            if cw is None:  # what the context's mode gives this track ({1, 1} on at most two channels: the plain path)
                if not layout and len(t.channels) > 2:
                    raise ValueError("in pair mode a track of more than two channels cannot share a call with weighted tracks")
                cw = r128_layout_weights(len(t.channels)) if layout else [1.0] * len(t.channels)
            for k, v in enumerate(cw):
                weights[i].w[k] = v
        n_albums = len(first) - 1 if first is not None else 0
        album_first = (C.c_size_t * (n_albums + 1))(*first) if first is not None else None
        out = (_capi.R128TrackResult * max(1, n))()
        alb = (_capi.R128AlbumResult * max(1, n_albums))()
        counts, z = self._r128_blocks(tracks) if return_blocks else (None, None)
        dyn = adyn = st = st_counts = None
        if dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            adyn = (_capi.R128Dynamics * max(1, n_albums))()
            st_counts, st = self._r128_blocks(tracks, True) if return_short_term else (None, None)
        self._check(self._lib.rg_r128_analyze_pcm_weighted(
            self._ctx, descs, weights, n, album_first, n_albums, arena.ctypes.data, arena.nbytes, 0, int(true_peak), out, alb,
            z.ctypes.data if z is not None else None, dyn, adyn if first is not None else None,
            st.ctypes.data if st is not None else None))
        extra = ([_split_blocks(z, counts)] if return_blocks else []) + ([_split_blocks(st, st_counts)] if return_short_term else [])
        return out, alb, dyn, adyn, extra

    def _r128_blocks(self, tracks, short_term=False):
        count = self._lib.rg_r128_short_term_count if short_term else self._lib.rg_r128_block_count
        counts = [int(count(t.sample_rate, t.frames)) for t in tracks]
        return counts, np.zeros(max(1, sum(counts)), dtype=np.float64)

    def analyze_tracks_r128(self, tracks: Sequence[PcmTrack], true_peak: bool = False, return_blocks: bool = False,
                            dynamics: bool = False, return_short_term: bool = False):
        """Integrated loudness (BS.1770), gain to -18 LUFS, sample peak and optionally true peak of each track.
        return_blocks: also every track's gating-block mean squares (a list of float64 arrays).
        dynamics: every result carries an R128Dynamics (loudness range, momentary and short-term maxima).
        return_short_term (with dynamics): also every track's short-term block mean squares, after the gating blocks if both
        are asked for."""
        if return_short_term and not dynamics:
            raise ValueError("return_short_term needs dynamics=True")
        n = len(tracks)
        if any(t.channel_weights is not None for t in tracks):
            out, _, dyn, _, extra = self._r128_weighted(tracks, None, true_peak, return_blocks, dynamics, return_short_term)
            res = [_to_r128(out[i], tracks[i].file_type, dyn[i] if dyn is not None else None) for i in range(n)]
            return (res, *extra) if extra else res
        arena, descs = pack_tracks(tracks)
        out = (_capi.R128TrackResult * max(1, n))()
        counts, z = self._r128_blocks(tracks) if return_blocks else (None, None)
        zp = z.ctypes.data if z is not None else None
        dyn = None
        if dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            st_counts, st = self._r128_blocks(tracks, True) if return_short_term else (None, None)
            self._check(self._lib.rg_r128_analyze_pcm_batch_dynamics(self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, int(true_peak),
                                                                     out, zp, dyn, st.ctypes.data if st is not None else None))
        else:
            self._check(self._lib.rg_r128_analyze_pcm_batch(self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, int(true_peak), out, zp))
        res = [_to_r128(out[i], tracks[i].file_type, dyn[i] if dyn is not None else None) for i in range(n)]
        extra = ([_split_blocks(z, counts)] if return_blocks else []) + ([_split_blocks(st, st_counts)] if return_short_term else [])
        return (res, *extra) if extra else res

    def analyze_album_r128(self, tracks: Sequence[PcmTrack], true_peak: bool = False, return_blocks: bool = False,
                           dynamics: bool = False, return_short_term: bool = False):
        """The tracks, and the album: both gates over the union of the tracks' blocks.  dynamics, return_short_term: as in
        analyze_tracks_r128; the album's R128Dynamics is over the union of the tracks' short-term blocks."""
        if return_short_term and not dynamics:
            raise ValueError("return_short_term needs dynamics=True")
        n = len(tracks)
        if any(t.channel_weights is not None for t in tracks):
            out, alb, dyn, adyn, extra = self._r128_weighted(tracks, [0, n], true_peak, return_blocks, dynamics, return_short_term)
            res = _to_r128_album([_to_r128(out[i], tracks[i].file_type, dyn[i] if dyn is not None else None) for i in range(n)],
                                 alb[0], adyn[0] if adyn is not None else None)
            return (res, *extra) if extra else res
        arena, descs = pack_tracks(tracks)
        out = (_capi.R128TrackResult * max(1, n))()
        alb = _capi.R128AlbumResult()
        counts, z = self._r128_blocks(tracks) if return_blocks else (None, None)
        zp = z.ctypes.data if z is not None else None
        dyn = adyn = None
        if dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            adyn = _capi.R128Dynamics()
            st_counts, st = self._r128_blocks(tracks, True) if return_short_term else (None, None)
            self._check(self._lib.rg_r128_analyze_album_pcm_dynamics(self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, int(true_peak),
                                                                     out, C.byref(alb), zp, dyn, C.byref(adyn),
                                                                     st.ctypes.data if st is not None else None))
        else:
            self._check(self._lib.rg_r128_analyze_album_pcm(self._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, int(true_peak), out,
                                                            C.byref(alb), zp))
        res = _to_r128_album([_to_r128(out[i], tracks[i].file_type, dyn[i] if dyn is not None else None) for i in range(n)], alb, adyn)
        extra = ([_split_blocks(z, counts)] if return_blocks else []) + ([_split_blocks(st, st_counts)] if return_short_term else [])
        return (res, *extra) if extra else res

    def analyze_track_files_r128(self, files, true_peak: bool = False, track_index: Optional[int] = None, dynamics: bool = False) -> list:
        """analyze_track_files on the R 128 path: per file an R128Result, or the ReplayGainError it failed with."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.R128TrackResult * max(1, n))()
        status = (C.c_int32 * max(1, n))()
        ti = -1 if track_index is None else int(track_index)
        dyn = None
        if dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            self._check(self._lib.rg_r128_analyze_tracks_dynamics(self._ctx, paths, n, ti, int(true_peak), out, status, dyn))
        else:
            self._check(self._lib.rg_r128_analyze_tracks(self._ctx, paths, n, ti, int(true_peak), out, status))
        return [_to_r128(out[i], AudioFileType.Mp3, dyn[i] if dyn is not None else None) if status[i] == 0 else
                ReplayGainError(int(status[i]), self._lib.rg_tracks_error(self._ctx, i).decode("utf-8", "replace")) for i in range(n)]

    def analyze_album_files_r128(self, files, true_peak: bool = False, track_index: Optional[int] = None,
                                 dynamics: bool = False, timing: Optional[dict] = None) -> R128AlbumResult:
        """`timing`: as analyze_album_files."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.R128TrackResult * max(1, n))()
        alb = _capi.R128AlbumResult()
        ti = -1 if track_index is None else int(track_index)
        dyn = adyn = None
        t0 = time.perf_counter()
        if dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            adyn = _capi.R128Dynamics()
            rc = self._lib.rg_r128_analyze_album_dynamics(self._ctx, paths, n, ti, int(true_peak), out, C.byref(alb), dyn, C.byref(adyn))
        else:
            rc = self._lib.rg_r128_analyze_album(self._ctx, paths, n, ti, int(true_peak), out, C.byref(alb))
        if timing is not None:
            timing["c_call_seconds"] = time.perf_counter() - t0
        self._check(rc)
        return _to_r128_album([_to_r128(out[i], AudioFileType.Mp3, dyn[i] if dyn is not None else None) for i in range(n)], alb, adyn)

    def analyze_albums_r128(self, albums, true_peak: bool = False, dynamics: bool = False, return_blocks: bool = False,
                            return_short_term: bool = False):
        """analyze_album_r128 for every album of `albums` (a sequence of sequences of PcmTrack) as ONE call
        (rg_r128_analyze_albums_pcm[_dynamics]): one pass over all tracks, every album gated on the device in the same
        launches.  -> a list of R128AlbumResult, each bit for bit what analyze_album_r128 gives on that album's tracks;
        return_blocks / return_short_term: also, per album, the lists analyze_album_r128 returns."""
        if return_short_term and not dynamics:
            raise ValueError("return_short_term needs dynamics=True")
        tracks = [t for a in albums for t in a]
        first = [0]
        for a in albums:
            first.append(first[-1] + len(a))
        n, n_albums = len(tracks), len(albums)
        weighted = any(t.channel_weights is not None for t in tracks)
        if weighted:
            out, alb, dyn, adyn, wextra = self._r128_weighted(tracks, first, true_peak, return_blocks, dynamics, return_short_term)
            if return_blocks:
                z_split = wextra.pop(0)
            if return_short_term:
                st_split = wextra.pop(0)
        else:
            arena, descs = pack_tracks(tracks)
            album_first = (C.c_size_t * (n_albums + 1))(*first)
            out = (_capi.R128TrackResult * max(1, n))()
            alb = (_capi.R128AlbumResult * max(1, n_albums))()
            counts, z = self._r128_blocks(tracks) if return_blocks else (None, None)
            zp = z.ctypes.data if z is not None else None
            dyn = adyn = None
        if weighted:
            pass
        elif dynamics:
            dyn = (_capi.R128Dynamics * max(1, n))()
            adyn = (_capi.R128Dynamics * max(1, n_albums))()
            st_counts, st = self._r128_blocks(tracks, True) if return_short_term else (None, None)
            self._check(self._lib.rg_r128_analyze_albums_pcm_dynamics(self._ctx, descs, n, album_first, n_albums, arena.ctypes.data,
                                                                      arena.nbytes, 0, int(true_peak), out, alb, zp, dyn, adyn,
                                                                      st.ctypes.data if st is not None else None))
        else:
            self._check(self._lib.rg_r128_analyze_albums_pcm(self._ctx, descs, n, album_first, n_albums, arena.ctypes.data, arena.nbytes,
                                                             0, int(true_peak), out, alb, zp))
        res = [_to_r128_album([_to_r128(out[i], tracks[i].file_type, dyn[i] if dyn is not None else None)
                               for i in range(first[a], first[a + 1])], alb[a], adyn[a] if adyn is not None else None)
               for a in range(n_albums)]
        extra = []
        if return_blocks:
            zs = z_split if weighted else _split_blocks(z, counts)
            extra.append([zs[first[a]:first[a + 1]] for a in range(n_albums)])
        if return_short_term:
            ss = st_split if weighted else _split_blocks(st, st_counts)
            extra.append([ss[first[a]:first[a + 1]] for a in range(n_albums)])
        return (res, *extra) if extra else res

    def analyze_albums_files_r128(self, albums, true_peak: bool = False, track_index: Optional[int] = None,
                                  dynamics: bool = False, timing: Optional[dict] = None) -> list:
        """analyze_album_files_r128 for every album of `albums` (a sequence of file sequences) as ONE call
        (rg_r128_analyze_albums[_dynamics]).  -> per album an R128AlbumResult, or the ReplayGainError
        analyze_album_files_r128 would have raised for it.  `timing`: as analyze_album_files."""
        args = _albums_args_r128(albums, track_index, true_peak, dynamics)
        fn = self._lib.rg_r128_analyze_albums_dynamics if dynamics else self._lib.rg_r128_analyze_albums
        t0 = time.perf_counter()
        rc = fn(self._ctx, *args[:-1])
        if timing is not None:
            timing["c_call_seconds"] = time.perf_counter() - t0
        self._check(rc)
        return _albums_results_r128(args, lambda i: self._lib.rg_tracks_error(self._ctx, i))

    def find_peak_amplitude(self, track: PcmTrack) -> PeakAmplitudeResult:
        """find_peak_amplitude's scan over ALL channels (src/replaygain.rs:1210-1249)."""
        arena, descs = pack_tracks([track])
        pk = _capi.PeakResult()
        self._check(self._lib.rg_find_peak_pcm(self._ctx, descs, arena.ctypes.data, arena.nbytes, 0, C.byref(pk)))
        return PeakAmplitudeResult(pk.peak, pk.peak_pcm, pk.sample_rate)

    # -- file level: the reference's public functions (src/replaygain.rs:929-941, 1033-1074, 1140-1249) ----
    def set_decoder_command(self, command_template: Optional[str]):
        """Command (run by /bin/sh, `{}` = quoted path) that writes a WAV stream to stdout for files that are
        not RIFF/WAVE, e.g. "ffmpeg -v error -i {} -f wav -c:a pcm_f32le -".  None = WAV files only."""
        self._check(self._lib.rg_set_decoder_command(self._ctx, command_template.encode() if command_template else None))

    def analyze_track_file(self, file_path, track_index: Optional[int] = None) -> ReplayGainResult:
        """analyze_track_with_index (src/replaygain.rs:935-941)."""
        out = _capi.TrackResult()
        self._check(self._lib.rg_analyze_track(self._ctx, os.fsencode(os.fspath(file_path)),
                                               -1 if track_index is None else int(track_index), C.byref(out)))
        return _to_result(out, out.file_type)

    def analyze_album_files(self, files, track_index: Optional[int] = None, timing: Optional[dict] = None) -> AlbumGainResult:
        """analyze_album_with_index (src/replaygain.rs:1044-1074).  `timing` (measurement tools): receives `c_call_seconds`, the
        duration of the C call rg_analyze_album alone -- what a caller over the C ABI waits for; building the path array and the
        result objects of this wrapper costs a few microseconds per file on top."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.TrackResult * max(1, n))()
        alb = _capi.AlbumResult()
        t0 = time.perf_counter()
        rc = self._lib.rg_analyze_album(self._ctx, paths, n, -1 if track_index is None else int(track_index), out, C.byref(alb))
        if timing is not None:
            timing["c_call_seconds"] = time.perf_counter() - t0
        self._check(rc)
        return AlbumGainResult([_to_result(out[i], out[i].file_type) for i in range(n)], alb.album_loudness_db,
                               alb.album_gain_db, alb.album_peak)

    def analyze_track_files(self, files, track_index: Optional[int] = None, timing: Optional[dict] = None) -> list:
        """analyze_track for every file, as ONE GPU batch (files loaded on all host cores).  -> per file a
        ReplayGainResult, or the ReplayGainError analyze_track_file would have raised for it.  `timing`: as analyze_album_files."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.TrackResult * max(1, n))()
        status = (C.c_int32 * max(1, n))()
        t0 = time.perf_counter()
        rc = self._lib.rg_analyze_tracks(self._ctx, paths, n, -1 if track_index is None else int(track_index), out, status)
        if timing is not None:
            timing["c_call_seconds"] = time.perf_counter() - t0
        self._check(rc)
        res = []
        for i in range(n):
            if status[i] == 0:
                res.append(_to_result(out[i], out[i].file_type))
            else:
                res.append(ReplayGainError(int(status[i]), self._lib.rg_tracks_error(self._ctx, i).decode("utf-8", "replace")))
        return res

    def analyze_albums_files(self, albums, track_index: Optional[int] = None, timing: Optional[dict] = None) -> list:
        """analyze_album_files for every album of `albums` (a sequence of file sequences), as ONE call (rg_analyze_albums: the
        files of all albums loaded, decoded and analysed like analyze_track_files takes them).  -> per album an AlbumGainResult,
        or the ReplayGainError analyze_album_files would have raised for it.  `timing`: as analyze_album_files."""
        args = _albums_args(albums, track_index)
        t0 = time.perf_counter()
        rc = self._lib.rg_analyze_albums(self._ctx, *args[:-1])
        if timing is not None:
            timing["c_call_seconds"] = time.perf_counter() - t0
        self._check(rc)
        return _albums_results(args, lambda i: self._lib.rg_tracks_error(self._ctx, i))

    def find_peak_amplitude_file(self, file_path) -> PeakAmplitudeResult:
        pk = _capi.PeakResult()
        self._check(self._lib.rg_find_peak_amplitude(self._ctx, os.fsencode(os.fspath(file_path)), C.byref(pk)))
        return PeakAmplitudeResult(pk.peak, pk.peak_pcm, pk.sample_rate)

    def decode_mp3_device(self, data: bytes):
        """The split MP3 decoder (stage A on the host, stages B-E on this GPU) -> (float32 [channels][frames], StreamInfo);
        bit for bit what mp3dec.decode returns."""
        from . import mp3dec

        info = mp3dec.scan(data)
        cap = int(info.frames)
        out = np.zeros((int(info.channels), max(1, cap)), dtype=np.float32)
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        di = mp3dec.StreamInfo()
        self._check(self._lib.rg_mp3_decode_device(self._ctx, C.cast(buf, C.c_void_p), len(data), out[0].ctypes.data,
                                                   out[1].ctypes.data if info.channels == 2 else None, cap, C.byref(di)))
        return out[:, :int(di.frames)], di

    def decode_flac_device(self, data: bytes):
        """A FLAC stream through the device decoder (frame check, layout, decode kernels) -> (int32 [channels][samples],
        FlacInfo); bit for bit what flacdec.decode returns."""
        from . import flacdec

        L = flacdec._lib()
        _, info = flacdec.index(data)
        cap = int(info.frames)
        out = np.zeros((int(info.channels), max(1, cap)), dtype=np.int32)
        planes = (C.c_void_p * int(info.channels))(*[out[c].ctypes.data for c in range(int(info.channels))])
        di = flacdec.FlacInfo()
        self._check(L.rg_flac_decode_device(self._ctx, flacdec._buf(data), len(data), planes, cap, C.byref(di)))
        return out[:, :int(di.frames)], di

    def stage_flac_device(self, streams: Sequence[bytes]):
        """FLAC streams in memory through the file route's loading and staging (rg_flac_stage_device_batch: tuning key 14
        picks the device or the host decoder) -> (the arena as a uint8 array, [TrackDesc], [FlacInfo]): plane c of stream
        i is arena[descs[i].offset_bytes + c * descs[i].frames * element size ...], int16 for S16 planar, int32 for S32."""
        from . import flacdec

        L = flacdec._lib()
        n = len(streams)
        bufs = [flacdec._buf(s) for s in streams]
        ptrs = (C.c_void_p * max(1, n))(*[C.addressof(b) for b in bufs])
        lens = (C.c_size_t * max(1, n))(*[len(s) for s in streams])
        cap = 16
        for s in streams:  # what the arena is laid out for: every walked frame, each stream rounded up to 16 bytes
            info = flacdec.index(s)[1]
            cap += (int(info.frames) * int(info.channels) * (2 if info.bits_per_sample <= 16 else 4) + 15) // 16 * 16
        arena = np.zeros(cap, dtype=np.uint8)
        descs = (_capi.TrackDesc * max(1, n))()
        infos = (flacdec.FlacInfo * max(1, n))()
        used = C.c_size_t()
        self._check(L.rg_flac_stage_device_batch(self._ctx, n, ptrs, lens, descs, infos, arena.ctypes.data, arena.size, C.byref(used)))
        return arena[:used.value], list(descs[:n]), list(infos[:n])

    def flac_md5_arena(self, route: int, descs, bps, arena):
        """rg_flac_md5_arena, the seam of the FLAC MD5 kernel: the streams `descs` describe in the host arena `arena` ->
        [digest bytes]; route 0 = the host twin, route 1 = the arena copied to this GPU and hashed by the kernel."""
        from . import flacdec

        try:
            return flacdec.md5_arena(self._ctx, route, descs, bps, arena)
        except flacdec.FlacError as e:
            raise ReplayGainError(e.code, self._lib.rg_last_error(self._ctx).decode()) from None

    def verify_flac(self, files) -> list:
        """rg_flac_verify: every file decoded by the route the analysis uses and its PCM's MD5 compared with STREAMINFO's
        signature -> [FlacVerifyResult]; a file that cannot be decoded carries its ReplayGainError in `.error`."""
        from . import flacdec

        n = len(files)
        paths, out = self._file_args(files, flacdec.FlacVerifyRecord)
        self._check(flacdec._lib().rg_flac_verify(self._ctx, paths, n, out))
        return [FlacVerifyResult(bool(r.flags & flacdec.VERIFY_HAS_SIGNATURE), bool(r.flags & flacdec.VERIFY_MD5_MATCH),
                                 bool(r.flags & flacdec.VERIFY_LENGTH_MATCH), bool(r.flags & flacdec.VERIFY_COMPLETE),
                                 int(r.frames), int(r.total_samples), int(r.audio_frames), int(r.dropped_frames),
                                 bytes(r.md5_stream), bytes(r.md5_decoded), err) for r, err in self._file_records(out, n)]

    def verify_flac_raw(self, files) -> bytes:
        """verify_flac's rg_flac_verify_result array as the C call left it (tests compare routes byte for byte)."""
        from . import flacdec

        n = len(files)
        paths, out = self._file_args(files, flacdec.FlacVerifyRecord)
        self._check(flacdec._lib().rg_flac_verify(self._ctx, paths, n, out))
        return bytes(out)[:n * C.sizeof(flacdec.FlacVerifyRecord)]

    @staticmethod
    def _rip_flags(n: int, disc, flags):
        if flags is not None:
            if len(flags) != n:
                raise ValueError("flags: one entry per file")
            return [int(f) for f in flags]
        out = [0] * n
        if disc and n:
            out[0] |= _capi.RIP_FIRST_TRACK
            out[-1] |= _capi.RIP_LAST_TRACK
        return out

    def _rip_call(self, files, disc, flags):
        n = len(files)
        paths, out = self._file_args(files, _capi.RipRecord)
        fl = self._rip_flags(n, disc, flags)
        self._check(self._lib.rg_rip_checksums(self._ctx, paths, n, (C.c_uint32 * max(1, n))(*fl), out))
        return out, fl

    def _rip_results(self, out, fl, n):
        return [RipChecksums(int(r.crc32), int(r.crc32_nonnull), int(r.arv1), int(r.arv2), int(r.frames), int(r.null_samples),
                             int(r.sample_rate), int(r.dropped_frames), bool(r.flags & _capi.RIP_CD_RATE),
                             bool(r.flags & _capi.RIP_CD_FRAMES), bool(r.flags & _capi.RIP_COMPLETE),
                             bool(f & _capi.RIP_FIRST_TRACK), bool(f & _capi.RIP_LAST_TRACK), err)
                for (r, err), f in zip(self._file_records(out, n), fl)]

    def rip_checksums(self, files, disc: bool = True, flags=None) -> list:
        """rg_rip_checksums: `files` (16-bit stereo WAV or FLAC) decoded by the route the analysis uses and, from the PCM where
        it lies on this GPU, per file the CRC-32, the CRC-32 without null samples and the AccurateRip v1 / v2 signatures ->
        [RipChecksums].  disc=True takes the files as the tracks of one disc, in order: the first is flagged first, the last
        last (`flags`: RIP_FIRST_TRACK / RIP_LAST_TRACK per file instead).  A file that takes no part carries its
        ReplayGainError in `.error`."""
        out, fl = self._rip_call(files, disc, flags)
        return self._rip_results(out, fl, len(files))

    def rip_checksums_raw(self, files, disc: bool = True, flags=None) -> bytes:
        """rip_checksums' rg_rip_result array as the C call left it (tests compare routes byte for byte)."""
        out, _ = self._rip_call(files, disc, flags)
        return bytes(out)[:len(files) * C.sizeof(_capi.RipRecord)]

    def _rip_offsets_call(self, files, disc, flags, radius):
        n = len(files)
        paths, out = self._file_args(files, _capi.RipRecord)
        fl = self._rip_flags(n, disc, flags)
        width = 2 * max(0, min(int(radius), _capi.RIP_OFFSET_MAX)) + 1
        v1, v2 = np.full((n, width), 0xA5A5A5A5, dtype=np.uint32), np.full((n, width), 0xA5A5A5A5, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        rc = self._lib.rg_rip_offset_signatures(self._ctx, paths, n, (C.c_uint32 * max(1, n))(*fl), int(radius), out, v1.ctypes.data_as(u32p),
                                                v2.ctypes.data_as(u32p))
        return rc, out, v1, v2, fl

    def rip_offset_signatures_raw(self, files, disc: bool = True, flags=None, radius: int = _capi.RIP_OFFSET_MAX):
        """rg_rip_offset_signatures as the C call left its arrays -> (status, records' bytes, arv1, arv2): nothing is raised,
        so that a refused call's records and tables can be looked at."""
        rc, out, v1, v2, _ = self._rip_offsets_call(files, disc, flags, radius)
        return rc, bytes(out)[:len(files) * C.sizeof(_capi.RipRecord)], v1, v2

    def rip_offset_signatures(self, files, disc: bool = True, flags=None, radius: int = _capi.RIP_OFFSET_MAX) -> RipOffsetSignatures:
        """rg_rip_offset_signatures: the files are the tracks of one disc, in order (`disc`, `flags`: as rip_checksums); per
        track the AccurateRip v1 / v2 signatures at every sample offset -radius .. radius, computed on this GPU from the one
        decode that also gives `.tracks`, the rip_checksums results -> RipOffsetSignatures.  Raises ReplayGainError
        (RG_ERR_REFUSED) when a file takes no part or the disc does not fit the device at once."""
        rc, out, v1, v2, fl = self._rip_offsets_call(files, disc, flags, radius)
        self._check(rc)
        return RipOffsetSignatures(self._rip_results(out, fl, len(files)), int(radius), v1, v2)

    def rip_offsets_arena(self, route: int, descs, flags, radius: int, arena, want=(True, True)):
        """rg_rip_offsets_arena, the seam of the offsets kernel: the disc `descs` describe in the host arena `arena` ->
        (arv1, arv2) [n, 2 radius + 1]; route 0 = the definition on the host, route 1 = the arena copied to this GPU and the
        kernel, route 2 = arv1 by the sliding recurrence on the host (want=(True, False))."""
        return rip_offsets_arena(self._ctx, route, descs, flags, radius, arena, want)

    @staticmethod
    def rip_offsets_kernel_shape():
        return rip_offsets_kernel_shape()

    def rip_checksums_arena(self, route: int, descs, flags, arena):
        """rg_rip_checksums_arena, the seam of the rip checksum kernels: the tracks `descs` describe in the host arena `arena`
        -> [RipRecord]; route 0 = the serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the
        kernels' fold arithmetic on the host."""
        return rip_checksums_arena(self._ctx, route, descs, flags, arena)

    def _pcm_stats_call(self, files, min_clip_run, min_zero_run):
        paths, out = self._file_args(files, _capi.PcmStatsRecord)
        self._check(self._lib.rg_pcm_stats(self._ctx, paths, len(files), _stats_opts(min_clip_run, min_zero_run), out))
        return out

    def pcm_stats(self, files, min_clip_run: int = _capi.STATS_MIN_CLIP_RUN, min_zero_run: int = _capi.STATS_MIN_ZERO_RUN) -> list:
        """rg_pcm_stats: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where it
        lies on this GPU, per channel the clipped samples and clip runs, the zero runs inside the audio and at its edges, the DC
        sum, the bits in use, minimum and maximum -> [PcmStats].  A file that takes no part carries its ReplayGainError in
        `.error`."""
        out = self._pcm_stats_call(files, min_clip_run, min_zero_run)
        return [pcm_stats_from_record(r, err) for r, err in self._file_records(out, len(files))]

    def pcm_stats_raw(self, files, min_clip_run=None, min_zero_run=None) -> bytes:
        """pcm_stats' rg_pcm_stats_result array as the C call left it (tests compare routes byte for byte)."""
        out = self._pcm_stats_call(files, min_clip_run, min_zero_run)
        return bytes(out)[:len(files) * C.sizeof(_capi.PcmStatsRecord)]

    def pcm_stats_arena(self, route: int, descs, bits, arena, min_clip_run=None, min_zero_run=None):
        """rg_pcm_stats_arena, the seam of the stats kernels: the tracks `descs` describe in the host arena `arena` ->
        [PcmStatsRecord]; route 0 = the serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the
        kernels' chunking and fold arithmetic on the host."""
        return pcm_stats_arena(self._ctx, route, descs, bits, arena, min_clip_run, min_zero_run)

    @staticmethod
    def pcm_stats_kernel_shape():
        return pcm_stats_kernel_shape()

    def _dr_call(self, files, block_frames, top_permille):
        paths, out = self._file_args(files, _capi.DrRecord)
        self._check(self._lib.rg_dynamic_range(self._ctx, paths, len(files), _dr_opts(block_frames, top_permille), out))
        return out

    def dynamic_range(self, files, block_frames=None, top_permille=None) -> list:
        """rg_dynamic_range: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where
        it lies on this GPU, per channel the mean square and the peak of every 3-second block, the loudest fifth of the blocks
        and the second-highest block peak, and from them the DR figure -> [DynamicRange].  A file that takes no part carries its
        ReplayGainError in `.error`."""
        out = self._dr_call(files, block_frames, top_permille)
        return [dynamic_range_from_record(r, err) for r, err in self._file_records(out, len(files))]

    def dynamic_range_raw(self, files, block_frames=None, top_permille=None) -> bytes:
        """dynamic_range's rg_dr_result array as the C call left it (tests compare routes byte for byte)."""
        out = self._dr_call(files, block_frames, top_permille)
        return bytes(out)[:len(files) * C.sizeof(_capi.DrRecord)]

    def dr_arena(self, route: int, descs, arena, block_frames=None, top_permille=None):
        """rg_dr_arena, the seam of the DR kernels: the tracks `descs` describe in the host arena `arena` -> [DrRecord]; route 0
        = the serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the kernels' cutting and fold
        arithmetic on the host."""
        return dr_arena(self._ctx, route, descs, arena, block_frames, top_permille)

    @staticmethod
    def dr_kernel_shape(fmt: int):
        return dr_kernel_shape(fmt)

    def _stereo_call(self, files, radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit, lag_sums):
        paths, out = self._file_args(files, _capi.StereoRecord)
        rows, rows_p = _stereo_rows(len(files), radius, lag_sums)
        opts = _stereo_opts(radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit)
        self._check(self._lib.rg_stereo(self._ctx, paths, len(files), opts, out, rows_p))
        return out, rows

    def stereo(self, files, radius=None, block_frames=None, phase_permille=None, delay_permille=None, mono_db=None, balance_db_limit=None,
               lag_sums=False):
        """rg_stereo: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where it
        lies on this GPU, the moments of channels 0 and 1 per block, the raw comparisons and the cross-correlation at every lag
        within `radius` -> [StereoImage], or with `lag_sums` ([StereoImage], int64 array of one row of 2 * radius + 1 sums per
        file).  A file that takes no part carries its ReplayGainError in `.error`."""
        out, rows = self._stereo_call(files, radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit, lag_sums)
        recs = [stereo_from_record(r, err) for r, err in self._file_records(out, len(files))]
        return (recs, rows[:len(files)]) if lag_sums else recs

    def stereo_raw(self, files, radius=None, block_frames=None, lag_sums=False):
        """stereo's rg_stereo_result array as the C call left it, and with `lag_sums` the rows' bytes behind it (tests compare
        routes byte for byte)."""
        out, rows = self._stereo_call(files, radius, block_frames, None, None, None, None, lag_sums)
        raw = bytes(out)[:len(files) * C.sizeof(_capi.StereoRecord)]
        return (raw, rows[:len(files)].tobytes()) if lag_sums else raw

    def stereo_arena(self, route: int, descs, arena, radius=None, block_frames=None, phase_permille=None, delay_permille=None, mono_db=None,
                     balance_db_limit=None, lag_sums=False):
        """rg_stereo_arena, the seam of the stereo kernels: the tracks `descs` describe in the host arena `arena` ->
        [StereoRecord] (with `lag_sums`: and the rows); route 0 = the serial host twin, route 1 = the arena copied to this GPU and
        the kernels, route 2 = the kernels' cutting and fold arithmetic on the host."""
        return stereo_arena(self._ctx, route, descs, arena, radius, block_frames, phase_permille, delay_permille, mono_db, balance_db_limit, lag_sums)

    @staticmethod
    def stereo_kernel_shape(fmt: int):
        return stereo_kernel_shape(fmt)

    def encode_flac(self, files, out_files, block_size=None, max_lpc_order=None, verify=True) -> list:
        """rg_flac_encode_files: `files` (WAV with integer samples, FLAC) decoded by the route the analysis uses and encoded
        where their PCM lies on this GPU, files[i] into out_files[i] -> [FlacEncoded].  With `verify` every stream is decoded
        again by the device decoder and its MD5 held to the source's before the file is written.  A file that fails carries its
        ReplayGainError in `.error` and leaves no output."""
        if len(files) != len(out_files):
            raise ValueError("encode_flac: as many outputs as inputs")
        n = len(files)
        paths, out = self._file_args(files, _capi.FlacEncodeRecord)
        outs = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in out_files])
        self._check(self._lib.rg_flac_encode_files(self._ctx, paths, outs, n, _flac_encode_opts(block_size, max_lpc_order, verify), out))
        return [FlacEncoded(int(r.pcm_frames), int(r.flac_frames), int(r.dropped_frames), int(r.sample_rate), int(r.channels), int(r.bits_per_sample),
                            int(r.block_size), int(r.min_frame_bytes), int(r.max_frame_bytes), int(r.pcm_bytes), int(r.stream_bytes),
                            int(r.metadata_bytes), bytes(r.md5_pcm), bytes(r.md5_decoded), int(r.flags), err) for r, err in self._file_records(out, n)]

    def flac_encode_arena(self, route: int, descs, bps, arena, block_size=None, max_lpc_order=None):
        """rg_flac_encode_arena, the seam of the FLAC encoder: the tracks `descs` describe in the host arena `arena` ->
        ([stream bytes], [FlacEncodeRecord], offsets); route 0 = the serial host twin, route 1 = the arena copied to this GPU
        and the analyse, layout and write kernels."""
        return flac_encode_arena(self._ctx, route, descs, bps, arena, block_size, max_lpc_order)

    def _compare_call(self, files, pairs, hints, blocks_per_pair, lag_sums, opts):
        n = len(files)
        if pairs is None:
            pairs = [(0, j) for j in range(1, n)]  # every file against the first
        if hints is not None:
            hints = [int(hints)] * len(pairs) if np.isscalar(hints) else [int(h) for h in hints]
            if len(hints) != len(pairs):
                raise ValueError("compare: as many hints as pairs")
            opts = dict(opts, align=_capi.CMP_ALIGN_HINT)
        n_pairs = len(pairs)
        paths, _ = self._file_args(files, _capi.CompareRecord)
        pr = (_capi.ComparePair * max(1, n_pairs))(*[_capi.ComparePair(int(p[0]), int(p[1]), hints[k] if hints is not None else 0) for k, p in enumerate(pairs)])
        out = (_capi.CompareRecord * max(1, n_pairs))()
        o, o_p = _compare_opts(**opts)
        per = max(0, int(blocks_per_pair))
        blocks = (_capi.CompareBlock * max(1, n_pairs * per))() if per else None
        rows = np.zeros((max(1, n_pairs), max(1, min(o.segments, _capi.CMP_MAX_SEGMENTS)), _capi.CMP_MAX_CHANNELS,
                         2 * min(o.radius, _capi.CMP_MAX_RADIUS) + 3), dtype=np.int64) if lag_sums else None
        self._check(self._lib.rg_compare(self._ctx, paths, n, pr, n_pairs, o_p, out, blocks, per, rows.ctypes.data_as(C.POINTER(C.c_int64)) if lag_sums else None))
        return pairs, out, blocks, rows

    def compare(self, files, pairs=None, hints=None, radius=None, blocks_per_pair=0, lag_sums=False, **opts) -> list:
        """rg_compare, a null test: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, where the PCM
        lies on this GPU, copy b of every pair lined up with the reference copy a to the sample, one gain fitted, and what is left
        sized -> [Comparison], one per pair.  `pairs`: (a, b) indices into `files`, None = every file against the first.  `hints`:
        None = the coarse lag comes from the fingerprint match; a number or one per pair = the expected lag in frames
        (b[n + hint] beside a[n]).  With `blocks_per_pair` > 0 also, per pair, its first CompareBlock rows; with `lag_sums` also
        the lag rows, an int64 array [pair][segment][channel (8)][2 * radius + 3].  A pair one of whose files fails carries that
        file's ReplayGainError in `.error`."""
        pairs, out, blocks, rows = self._compare_call(files, pairs, hints, blocks_per_pair, lag_sums, dict(opts, radius=radius))
        recs = []
        for k, p in enumerate(pairs):
            err = None
            if out[k].status != 0:
                texts = [self._lib.rg_compare_error(self._ctx, k).decode("utf-8", "replace")]  # the pair's own text, then its files'
                texts += [self._lib.rg_tracks_error(self._ctx, int(i)).decode("utf-8", "replace") for i in p[:2]]
                err = ReplayGainError(int(out[k].status), next((t for t in texts if t), "not compared"))
            recs.append(compare_from_record(out[k], err))
        res = [recs]
        if blocks_per_pair:
            res.append([[blocks[k * blocks_per_pair + j] for j in range(min(blocks_per_pair, out[k].blocks))] for k in range(len(pairs))])
        if lag_sums:
            res.append(rows[:len(pairs)])
        return res[0] if len(res) == 1 else tuple(res)

    def compare_raw(self, files, pairs=None, hints=None, blocks_per_pair=0, **opts):
        """compare's rg_compare_result array as the C call left it, then the block rows' and the lag rows' bytes (tests compare
        routes byte for byte)."""
        pairs, out, blocks, rows = self._compare_call(files, pairs, hints, blocks_per_pair, True, opts)
        return bytes(out)[:len(pairs) * C.sizeof(_capi.CompareRecord)], bytes(blocks) if blocks is not None else b"", rows[:len(pairs)].tobytes()

    def compare_arena(self, route: int, descs, pairs, arena, blocks_per_pair=0, lag_sums=False, **opts):
        """rg_compare_arena, the seam of the null-test kernels: the pairs (a, b, hint) of the tracks `descs` describe in the host
        arena `arena` -> [CompareRecord] (with `blocks_per_pair` / `lag_sums`: and the block rows / the lag rows); route 0 = the
        serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the kernels' cutting on the host."""
        return compare_arena(self._ctx, route, descs, pairs, arena, blocks_per_pair, lag_sums, **opts)

    @staticmethod
    def compare_kernel_shape(fmt_a: int, fmt_b: int = None):
        return compare_kernel_shape(fmt_a, fmt_b)

    def _clicks_call(self, files, block_samples, order, ratio_permille, floor, gap, max_width, max_events):
        paths, out = self._file_args(files, _capi.ClicksRecord)
        k, rows = _clicks_rows(len(files), max_events)
        opts = _clicks_opts(block_samples, order, ratio_permille, floor, gap, max_width, max_events)
        self._check(self._lib.rg_clicks(self._ctx, paths, len(files), opts, out, rows))
        return out, rows, k

    def clicks(self, files, block_samples=None, order=None, ratio_permille=None, floor=None, gap=None, max_width=None, max_events=None):
        """rg_clicks: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where it lies
        on this GPU, every channel predicted block by block by the FLAC encoder's linear model; samples whose residual stands
        `ratio_permille` / 1000 times above the median residual around them make events, narrow events are clicks -> [Clicks],
        each with its channels and the file's first `max_events` events.  A file that takes no part carries its ReplayGainError in
        `.error`."""
        out, rows, k = self._clicks_call(files, block_samples, order, ratio_permille, floor, gap, max_width, max_events)
        return [clicks_from_record(r, rows[i * k:(i + 1) * k], err) for i, (r, err) in enumerate(self._file_records(out, len(files)))]

    def clicks_raw(self, files, block_samples=None, order=None, ratio_permille=None, max_events=None):
        """clicks' rg_clicks_result array as the C call left it, and the event rows' bytes behind it (tests compare routes byte for
        byte)."""
        out, rows, k = self._clicks_call(files, block_samples, order, ratio_permille, None, None, None, max_events)
        return bytes(out)[:len(files) * C.sizeof(_capi.ClicksRecord)], bytes(rows)[:len(files) * k * C.sizeof(_capi.ClicksEvent)]

    def clicks_arena(self, route: int, descs, arena, block_samples=None, order=None, ratio_permille=None, floor=None, gap=None, max_width=None,
                     max_events=None):
        """rg_clicks_arena, the seam of the click kernels: the tracks `descs` describe in the host arena `arena` -> ([ClicksRecord],
        the event rows); route 0 = the serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the
        kernels' tile and fold code on one host lane."""
        return clicks_arena(self._ctx, route, descs, arena, block_samples, order, ratio_permille, floor, gap, max_width, max_events)

    @staticmethod
    def clicks_kernel_shape(block_samples: int):
        return clicks_kernel_shape(block_samples)

    def _same_recording_call(self, files, block, probes, radius, max_ber_permille, codes_cap):
        paths, out = self._file_args(files, _capi.FingerprintRecord)
        n = len(files)
        max_pairs = n * (n - 1) // 2
        pairs = (_capi.FingerprintPair * max(1, max_pairs))()
        n_pairs = C.c_size_t(0)
        codes = np.zeros(max(1, int(codes_cap)), dtype=np.uint32) if codes_cap else None
        self._check(self._lib.rg_same_recording(self._ctx, paths, n, _fingerprint_opts(block, probes, radius, max_ber_permille), out, pairs, max_pairs,
                                                C.byref(n_pairs), codes.ctypes.data_as(C.POINTER(C.c_uint32)) if codes_cap else None,
                                                int(codes_cap) if codes_cap else 0))
        return out, pairs, int(n_pairs.value), codes

    def same_recording(self, files, block=None, probes=None, radius=None, max_ber_permille=None):
        """rg_same_recording: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses, fingerprinted where
        the PCM lies, and every pair matched at every lag within `radius` codes, all on this GPU ->
        ([Fingerprint], [SamePair], groups): the matching pairs in (i, j) order, and `groups` the lists of indices of the
        files that are the same recording (more than one file each), in order of their first file.  A file that takes no part
        carries its ReplayGainError in `.error`."""
        out, pairs, n_pairs, _ = self._same_recording_call(files, block, probes, radius, max_ber_permille, 0)
        recs = [fingerprint_from_record(r, err) for r, err in self._file_records(out, len(files))]
        found = [SamePair(int(p.i), int(p.j), int(p.errors), int(p.bits), int(p.lag), int(p.flags)) for p in pairs[:n_pairs]]
        by = {}
        for i, r in enumerate(recs):
            if r.error is None:
                by.setdefault(r.group, []).append(i)
        return recs, found, [g for _, g in sorted(by.items()) if len(g) > 1]

    def same_recording_raw(self, files, block=None, probes=None, radius=None, max_ber_permille=None, codes_cap=0):
        """same_recording's arrays as the C call left them -> (record bytes, pair bytes, codes or None): tests compare routes byte
        for byte."""
        out, pairs, n_pairs, codes = self._same_recording_call(files, block, probes, radius, max_ber_permille, codes_cap)
        return (bytes(out)[:len(files) * C.sizeof(_capi.FingerprintRecord)], bytes(pairs)[:n_pairs * C.sizeof(_capi.FingerprintPair)], codes)

    def _same_recording_any_rate_call(self, files, block, probes, radius, max_ber_permille, codes_cap):
        paths, out = self._file_args(files, _capi.XrateRecord)
        n = len(files)
        max_pairs = n * (n - 1) // 2
        pairs = (_capi.FingerprintPair * max(1, max_pairs))()
        n_pairs = C.c_size_t(0)
        codes = np.zeros(max(1, int(codes_cap)), dtype=np.uint32) if codes_cap else None
        self._check(self._lib.rg_same_recording_xrate(self._ctx, paths, n, _fingerprint_opts(block, probes, radius, max_ber_permille), out, pairs,
                                                      max_pairs, C.byref(n_pairs), codes.ctypes.data_as(C.POINTER(C.c_uint32)) if codes_cap else None,
                                                      int(codes_cap) if codes_cap else 0))
        return out, pairs, int(n_pairs.value), codes

    def same_recording_any_rate(self, files, block=None, probes=None, radius=None, max_ber_permille=None):
        """rg_same_recording_xrate: same_recording across sample rates.  Every file is brought to 11025 Hz on this GPU first (a
        rational polyphase resampler), fingerprinted there and matched with every other, whatever its own rate ->
        ([Fingerprint], [SamePair], groups) as same_recording gives them; `sample_rate` is the file's own, a code and a lag
        count 512 / 11025 s for every file, and None means this call's defaults (block 64, probes 8, radius 128)."""
        out, pairs, n_pairs, _ = self._same_recording_any_rate_call(files, block, probes, radius, max_ber_permille, 0)
        recs = [fingerprint_from_record(r, err) for r, err in self._file_records(out, len(files))]
        found = [SamePair(int(p.i), int(p.j), int(p.errors), int(p.bits), int(p.lag), int(p.flags)) for p in pairs[:n_pairs]]
        by = {}
        for i, r in enumerate(recs):
            if r.error is None:
                by.setdefault(r.group, []).append(i)
        return recs, found, [g for _, g in sorted(by.items()) if len(g) > 1]

    def same_recording_any_rate_raw(self, files, block=None, probes=None, radius=None, max_ber_permille=None, codes_cap=0):
        """same_recording_any_rate's arrays as the C call left them -> (record bytes, [XrateRecord], pair bytes, codes or None)."""
        out, pairs, n_pairs, codes = self._same_recording_any_rate_call(files, block, probes, radius, max_ber_permille, codes_cap)
        return (bytes(out)[:len(files) * C.sizeof(_capi.XrateRecord)], list(out[:len(files)]), bytes(pairs)[:n_pairs * C.sizeof(_capi.FingerprintPair)],
                codes)

    def resample_arena(self, route: int, descs, arena):
        """rg_resample_arena, the seam of the resampler -> ([ResampleRecord], y); route 0 = the definitions in double, route 1 =
        the arena copied to this GPU and the kernels, route 2 = the kernels' arithmetic on the host."""
        return resample_arena(self._ctx, route, descs, arena)

    def xrate_fingerprint_arena(self, route: int, descs, arena, bands=True):
        """rg_xrate_fingerprint_arena, the resampler and the fingerprint kernels on its output -> ([XrateRecord], codes, bands, y)."""
        return xrate_fingerprint_arena(self._ctx, route, descs, arena, bands)

    def fingerprint_arena(self, route: int, descs, arena, bands=True):
        """rg_fingerprint_arena, the seam of the fingerprint kernels -> ([FingerprintRecord], codes, bands); route 0 = the
        serial host twin, route 1 = the arena copied to this GPU and the kernels, route 2 = the kernels' arithmetic on the host."""
        return fingerprint_arena(self._ctx, route, descs, arena, bands)

    def fingerprint_match_codes(self, route: int, codes, rates, block=None, probes=None, radius=None, max_ber_permille=None):
        """rg_fingerprint_match_codes, the seam of the match kernel, on constructed codes -> the pair records."""
        return fingerprint_match_codes(self._ctx, route, codes, rates, block, probes, radius, max_ber_permille)

    @staticmethod
    def fingerprint_kernel_shape():
        return fingerprint_kernel_shape()

    def _tempo_call(self, files, window, hop, min_bpm, onsets_cap):
        paths, out = self._file_args(files, _capi.TempoRecord)
        onsets = np.zeros(max(1, int(onsets_cap)), dtype=np.uint16) if onsets_cap else None
        self._check(self._lib.rg_tempo(self._ctx, paths, len(files), _tempo_opts(window, hop, min_bpm), out,
                                       onsets.ctypes.data_as(C.POINTER(C.c_uint16)) if onsets_cap else None, int(onsets_cap) if onsets_cap else 0))
        return out, onsets

    def tempo(self, files, window=None, hop=None, min_bpm=None):
        """rg_tempo: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses; the onset curve, its windowed
        autocorrelation and the beat grid where the PCM lies, all on this GPU -> [Tempo].  A file that fails carries its
        ReplayGainError in `.error`."""
        out, _ = self._tempo_call(files, window, hop, min_bpm, 0)
        return [tempo_from_record(r, err) for r, err in self._file_records(out, len(files))]

    def tempo_raw(self, files, window=None, hop=None, min_bpm=None, onsets_cap=0):
        """tempo's arrays as the C call left them -> (record bytes, [TempoRecord], onsets or None): tests compare routes byte for
        byte."""
        out, onsets = self._tempo_call(files, window, hop, min_bpm, onsets_cap)
        return bytes(out)[:len(files) * C.sizeof(_capi.TempoRecord)], list(out[:len(files)]), onsets

    def tempo_arena(self, route: int, descs, arena, window=None, hop=None, min_bpm=None, bands=True):
        """rg_tempo_arena, the seam of the tempo kernels -> ([TempoRecord], onsets, bands); route 0 = the serial host twin,
        route 1 = the arena copied to this GPU and the kernels, route 2 = the kernels' arithmetic on the host."""
        return tempo_arena(self._ctx, route, descs, arena, window, hop, min_bpm, bands)

    def tempo_from_onsets(self, route: int, onsets, rates, window=None, hop=None, min_bpm=None):
        """rg_tempo_from_onsets, the seam of the window and finish kernels, on constructed curves -> ([TempoRecord], acf)."""
        return tempo_from_onsets(self._ctx, route, onsets, rates, window, hop, min_bpm)

    @staticmethod
    def tempo_kernel_shape():
        return tempo_kernel_shape()

    def _key_call(self, files, segment, chroma_cap):
        paths, out = self._file_args(files, _capi.KeyRecord)
        chroma = np.zeros((max(1, int(chroma_cap)), _capi.KEY_CHROMA), dtype=np.uint16) if chroma_cap else None
        self._check(self._lib.rg_key(self._ctx, paths, len(files), _key_opts(segment), out,
                                     chroma.ctypes.data_as(C.POINTER(C.c_uint16)) if chroma_cap else None, int(chroma_cap) if chroma_cap else 0))
        return out, chroma

    def key(self, files, segment=None):
        """rg_key: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses; the decimation, the chroma rows
        and the key-profile match where the PCM lies, all on this GPU -> [Key].  A file that fails carries its ReplayGainError
        in `.error`."""
        out, _ = self._key_call(files, segment, 0)
        return [key_from_record(r, err) for r, err in self._file_records(out, len(files))]

    def key_raw(self, files, segment=None, chroma_cap=0):
        """key's arrays as the C call left them -> (record bytes, [KeyRecord], chroma rows or None): tests compare routes byte
        for byte."""
        out, chroma = self._key_call(files, segment, chroma_cap)
        return bytes(out)[:len(files) * C.sizeof(_capi.KeyRecord)], list(out[:len(files)]), chroma

    def key_arena(self, route: int, descs, arena, segment=None, bands=True):
        """rg_key_arena, the seam of the key kernels -> ([KeyRecord], y, bands, chroma); route 0 = the serial host twin, route 1 =
        the arena copied to this GPU and the kernels, route 2 = the kernels' arithmetic on the host."""
        return key_arena(self._ctx, route, descs, arena, segment, bands)

    def key_from_chroma(self, route: int, chroma, segment=None):
        """rg_key_from_chroma, the seam of the finish kernel, on constructed rows -> [KeyRecord]."""
        return key_from_chroma(self._ctx, route, chroma, segment)

    @staticmethod
    def key_kernel_shape():
        return key_kernel_shape()

    def _ancestry_call(self, files, segments, granules, z_min, iso_min, active_floor):
        paths, out = self._file_args(files, _capi.AncestryRecord)
        self._check(self._lib.rg_ancestry(self._ctx, paths, len(files), _ancestry_opts(segments, granules, z_min, iso_min, active_floor), out))
        return out

    def ancestry(self, files, segments=None, granules=None, z_min=None, iso_min=None, active_floor=None) -> list:
        """rg_ancestry: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where it
        lies on this GPU, put through the MP3 encoder's hybrid filterbank at all 576 alignments, per channel (and mid and side of
        a stereo file): the alignment at which the most lines fall to zero, how far it stands out, and whether that is an MP3
        granule grid -> [Ancestry].  A file that takes no part carries its ReplayGainError in `.error`."""
        out = self._ancestry_call(files, segments, granules, z_min, iso_min, active_floor)
        return [ancestry_from_record(r, err) for r, err in self._file_records(out, len(files))]

    def ancestry_raw(self, files, segments=None, granules=None, z_min=None, iso_min=None, active_floor=None) -> bytes:
        """ancestry's rg_ancestry_result array as the C call left it (tests compare routes byte for byte)."""
        out = self._ancestry_call(files, segments, granules, z_min, iso_min, active_floor)
        return bytes(out)[:len(files) * C.sizeof(_capi.AncestryRecord)]

    def ancestry_arena(self, route: int, descs, arena, segments=None, granules=None, z_min=None, iso_min=None, active_floor=None, counts=True):
        """rg_ancestry_arena, the seam of the ancestry kernels: the tracks `descs` describe in the host arena `arena` ->
        ([AncestryRecord], counts); route 0 = the serial host twin, route 1 = the arena copied to this GPU and the kernels,
        route 2 = the kernels' cutting on the host."""
        return ancestry_arena(self._ctx, route, descs, arena, segments, granules, z_min, iso_min, active_floor, counts)

    @staticmethod
    def ancestry_kernel_shape():
        return ancestry_kernel_shape()

    def _spectrum_call(self, files, edge_db, min_cutoff_hz, bands):
        n = len(files)
        paths, out = self._file_args(files, _capi.SpectrumRecord)
        e = _spectrum_bands(n) if bands else None
        self._check(self._lib.rg_spectrum(self._ctx, paths, n, _spectrum_opts(edge_db, min_cutoff_hz), out,
                                          e.ctypes.data_as(C.POINTER(C.c_double)) if bands else None))
        return out, e

    def spectrum(self, files, edge_db=None, min_cutoff_hz=None, bands: bool = False) -> list:
        """rg_spectrum: `files` (WAV, FLAC or MPEG Layer III) decoded by the route the analysis uses and, from the PCM where it
        lies on this GPU, per channel the long-term power spectrum in 256 bands, the frequency above which there is nothing and
        the steepness of the edge there -> [Spectrum], with the band energies in every channel's `.bands` when `bands` is true.
        A file that takes no part carries its ReplayGainError in `.error`."""
        out, e = self._spectrum_call(files, edge_db, min_cutoff_hz, bands)
        return [spectrum_from_record(r, err, e[i] if bands else None) for i, (r, err) in enumerate(self._file_records(out, len(files)))]

    def spectrum_raw(self, files, edge_db=None, min_cutoff_hz=None):
        """spectrum's rg_spectrum_result array and band energies as the C call left them -> (bytes, bytes)."""
        out, e = self._spectrum_call(files, edge_db, min_cutoff_hz, True)
        return bytes(out)[:len(files) * C.sizeof(_capi.SpectrumRecord)], e[:len(files)].tobytes()

    def spectrum_arena(self, route: int, descs, arena, edge_db=None, min_cutoff_hz=None, bands=True):
        """rg_spectrum_arena, the seam of the spectrum kernels: the tracks `descs` describe in the host arena `arena` ->
        ([SpectrumRecord], E); route 0 = the serial host twin in double, route 1 = the arena copied to this GPU and the kernels,
        route 2 = the kernels' arithmetic on the host."""
        return spectrum_arena(self._ctx, route, descs, arena, edge_db, min_cutoff_hz, bands)

    @staticmethod
    def spectrum_kernel_shape():
        return spectrum_kernel_shape()

    @staticmethod
    def spectrum_verdict(p, analysed_frames, sample_rate, edge_db=None, min_cutoff_hz=None):
        return spectrum_verdict(p, analysed_frames, sample_rate, edge_db, min_cutoff_hz)

    def verify_mp3(self, files) -> list:
        """rg_mp3_verify: every file decoded by the route the analysis uses, its dropped frames counted, and the LAME music
        CRC, the info tag's CRC and the frame CRCs computed on this GPU -> [mp3verify.Mp3VerifyResult]; a file that is not a
        bare MPEG Layer III stream or cannot be opened carries its ReplayGainError in `.error`."""
        from . import mp3verify

        paths, out = self._file_args(files, mp3verify.Mp3VerifyRecord)
        self._check(mp3verify._lib().rg_mp3_verify(self._ctx, paths, len(files), out))
        return [mp3verify.result_of(r, err) for r, err in self._file_records(out, len(files))]

    def verify_mp3_raw(self, files) -> bytes:
        """verify_mp3's rg_mp3_verify_result array as the C call left it (tests compare routes byte for byte)."""
        from . import mp3verify

        n = len(files)
        paths, out = self._file_args(files, mp3verify.Mp3VerifyRecord)
        self._check(mp3verify._lib().rg_mp3_verify(self._ctx, paths, n, out))
        return bytes(out)[:n * C.sizeof(mp3verify.Mp3VerifyRecord)]

    def mp3_crc_ranges(self, route: int, offsets, lengths, data):
        """rg_mp3_crc_ranges, the seam of the CRC-16/ARC chunk and fold kernels (route 1) and their host twin (route 0)."""
        from . import mp3verify

        try:
            return mp3verify.crc_ranges(self._ctx, route, offsets, lengths, data)
        except mp3verify.Mp3VerifyError as e:
            raise ReplayGainError(e.code, self._lib.rg_last_error(self._ctx).decode()) from None

    def mp3_frame_crc_check(self, route: int, frame_offsets, data):
        """rg_mp3_frame_crc_check, the seam of the frame-CRC kernel (route 1) and its host twin (route 0)."""
        from . import mp3verify

        try:
            return mp3verify.frame_crc_check(self._ctx, route, frame_offsets, data)
        except mp3verify.Mp3VerifyError as e:
            raise ReplayGainError(e.code, self._lib.rg_last_error(self._ctx).decode()) from None

    def decode_mp3_bench(self, data: bytes, copies: int, reps: int = 5) -> dict:
        """rg_mp3_decode_bench: per-kernel HIP-event times of the device decode chain on `copies` copies of one stream."""
        ms = (C.c_double * 5)()
        units, cbytes, frames = C.c_uint64(), C.c_uint64(), C.c_uint64()
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        self._check(self._lib.rg_mp3_decode_bench(self._ctx, buf, len(data), copies, reps, ms, C.byref(units), C.byref(cbytes), C.byref(frames)))
        # chain_pipelined: per chunk in the file route's arrangement (frame parser and lane sort beside the chunk before)
        return {"ms": {"frames": ms[0], "huffman": ms[1], "backhalf": ms[2], "chain": ms[3], "chain_pipelined": ms[4]},
                "units": units.value, "compressed_bytes": cbytes.value, "frames": frames.value}

    def analyze_wav_bytes(self, wavs: Sequence[bytes], album: bool = False):
        """WAV streams already in memory -> [ReplayGainResult] (+ AlbumGainResult fields when album)."""
        n = len(wavs)
        keep = [C.c_char_p(bytes(w) if not isinstance(w, bytes) else w) for w in wavs]  # no copy: points into the bytes objects
        ptrs = (C.c_void_p * max(1, n))(*[C.cast(k, C.c_void_p).value for k in keep])
        lens = (C.c_size_t * max(1, n))(*[len(w) for w in wavs])
        out = (_capi.TrackResult * max(1, n))()
        alb = _capi.AlbumResult()
        self._check(self._lib.rg_analyze_wav_batch(self._ctx, ptrs, lens, n, int(album), out, C.byref(alb)))
        res = [_to_result(out[i], AudioFileType.Mp3) for i in range(n)]
        return AlbumGainResult(res, alb.album_loudness_db, alb.album_gain_db, alb.album_peak) if album else res

    # -- synchronous, PCM already resident on the device (one blocking call = the reference's API shape) ----
    def analyze_device(self, descs, n: int, d_pcm_base: int, pcm_bytes: int, want_hist: bool = False, out=None):
        """rg_analyze_pcm_batch with pcm_on_device = 1: ONE batch in flight, results (exact repeat of flagged tracks
        included) when the call returns.  With `out` (a ctypes TrackResult array) the raw records are left there and
        nothing is converted (timing loops)."""
        if out is not None:
            self._check(self._lib.rg_analyze_pcm_batch(self._ctx, descs, n, d_pcm_base, pcm_bytes, 1, out, None))
            return out
        out = (_capi.TrackResult * max(1, n))()
        hist = np.zeros((max(1, n), _capi.HISTOGRAM_SIZE), dtype=np.uint32) if want_hist else None
        self._check(self._lib.rg_analyze_pcm_batch(self._ctx, descs, n, d_pcm_base, pcm_bytes, 1, out,
                                                   hist.ctypes.data if hist is not None else None))
        res = [_to_result(out[i], AudioFileType.Mp3) for i in range(n)]
        return (res, hist[:n]) if want_hist else res

    # -- device-resident pipeline --------------------------------------------------------------
    def enqueue_device(self, descs, n: int, d_pcm_base: int, pcm_bytes: int, album: bool = False):
        self._check(self._lib.rg_enqueue_pcm_batch(self._ctx, descs, n, d_pcm_base, pcm_bytes, int(album)))

    def collect(self, n: int, want_hist: bool = False):
        out = (_capi.TrackResult * max(1, n))()
        hist = np.zeros((max(1, n), _capi.HISTOGRAM_SIZE), dtype=np.uint32) if want_hist else None
        self._check(self._lib.rg_collect(self._ctx, out, hist.ctypes.data if hist is not None else None))
        res = [_to_result(out[i], AudioFileType.Mp3) for i in range(n)]
        return (res, hist[:n]) if want_hist else res

    def collect_exact(self, descs, n: int, d_pcm_base: int, pcm_bytes: int, want_hist: bool = False):
        """collect() with the synchronous calls' guarantee: a batch that has a track flagged imprecise is run once more with
        that track on the order-faithful kernel (the PCM must still be in place)."""
        out = (_capi.TrackResult * max(1, n))()
        hist = np.zeros((max(1, n), _capi.HISTOGRAM_SIZE), dtype=np.uint32) if want_hist else None
        self._check(self._lib.rg_collect_exact(self._ctx, descs, n, d_pcm_base, pcm_bytes, out,
                                               hist.ctypes.data if hist is not None else None))
        res = [_to_result(out[i], AudioFileType.Mp3) for i in range(n)]
        return (res, hist[:n]) if want_hist else res

    def device_view(self) -> _capi.DeviceView:
        v = _capi.DeviceView()
        self._check(self._lib.rg_device_view_get(self._ctx, C.byref(v)))
        return v

    def album_allreduce(self, nccl_comm: Optional[int] = None):
        self._check(self._lib.rg_album_allreduce(self._ctx, nccl_comm))

    def album_reduce_gathered(self, d_gathered: int, world: int):
        self._check(self._lib.rg_album_reduce_gathered(self._ctx, d_gathered, world))

    # -- the library's own RCCL communicator (rg_comm_*): the exchange runs on the batch's stream -----------
    def comm_init(self, unique_id: bytes, world: int, rank: int):
        self._check(self._lib.rg_comm_init(self._ctx, unique_id, world, rank))

    def comm_init_torch(self, group=None, library: Optional[str] = None):
        """Bootstrap through torch.distributed: rank 0's ncclUniqueId is broadcast over the (already
        initialised) process group, then every rank joins.  torch's own librccl.so is the one used unless `library`
        (or the environment's MP3RGAIN_AMD_RCCL_LIBRARY) names another -- the tests' stand-in transport, which lets
        several ranks share one GPU (tests/standin_rccl).
        Every rank raises, or none does: failures are agreed on over the process group."""
        import torch
        import torch.distributed as dist

        lib = library or os.environ.get("MP3RGAIN_AMD_RCCL_LIBRARY") or os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        explicit = bool(library or os.environ.get("MP3RGAIN_AMD_RCCL_LIBRARY"))
        # a library named explicitly must exist and load: silently going on with whatever librccl.so resolves instead (real
        # RCCL where the stand-in was meant refuses two ranks on one device) would fail on some ranks only
        if os.path.exists(lib):
            lib_rc = self._lib.rg_comm_library(os.fsencode(lib))
        else:
            lib_rc = -1 if explicit else 0
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        src = dist.get_global_rank(group, 0) if group is not None else 0
        uid = b""
        if rank == 0:
            buf = C.create_string_buffer(_capi.COMM_ID_BYTES)
            if self._lib.rg_comm_unique_id(buf) == 0:
                uid = buf.raw
        box = [uid]
        dist.broadcast_object_list(box, src=src, group=group)
        if not box[0]:
            raise ReplayGainError(-7, "ncclGetUniqueId failed on rank 0 (librccl.so not found?)")
        err = None
        if explicit and lib_rc != 0:  # a library that was asked for by name and cannot be loaded: agreed on below, like any other failure
            err = ReplayGainError(int(lib_rc), f"refused {lib}: not a librccl.so[.N] (a stand-in transport needs MP3RGAIN_AMD_TEST_SEAMS=1)"
                                  if int(lib_rc) == -10 else f"cannot load {lib}")
        else:
            try:
                self.comm_init(box[0], world, rank)
            except ReplayGainError as ex:
                err = ex
        flags = [None] * world
        dist.all_gather_object(flags, err is None, group=group)
        if not all(flags):
            self.comm_destroy()
            raise err or ReplayGainError(-7, "ncclCommInitRank failed on another rank")

    def comm_info(self) -> dict:
        """{"ranks": ranks of the context's communicator (0 = none), "nccl_version": ncclGetVersion of the library behind it}"""
        w, v = C.c_int(0), C.c_int(0)
        self._check(self._lib.rg_comm_info(self._ctx, C.byref(w), C.byref(v)))
        return {"ranks": int(w.value), "nccl_version": int(v.value)}

    def comm_destroy(self):
        self._check(self._lib.rg_comm_destroy(self._ctx))

    def album_exchange(self):
        """Sum of histograms / max of peaks across the communicator's ranks, on the batch's stream."""
        self._check(self._lib.rg_album_exchange(self._ctx))

    def album_result_enqueue(self):
        self._check(self._lib.rg_album_result_enqueue(self._ctx))

    def album_finish(self, want_hist: bool = False):
        alb = _capi.AlbumResult()
        hist = np.zeros(_capi.HISTOGRAM_SIZE, dtype=np.uint32) if want_hist else None
        self._check(self._lib.rg_album_finish(self._ctx, C.byref(alb), hist.ctypes.data if hist is not None else None))
        return (alb, hist) if want_hist else alb

    def synth_fill_device(self, d_dst: int, seed: int, channel: int, sample_rate: int, first_frame: int, frames: int):
        self._check(self._lib.rg_synth_fill_device(self._ctx, d_dst, seed, channel, sample_rate, first_frame, frames))

    def timing_enable(self, on: bool = True):
        self._check(self._lib.rg_timing_enable(self._ctx, int(on)))

    def timing_read(self, reset: bool = True):
        """-> (sum of kernel durations [ms], launches, first-start-to-last-end span [ms])"""
        s, k, sp = C.c_double(), C.c_uint64(), C.c_double()
        self._check(self._lib.rg_timing_read(self._ctx, C.byref(s), C.byref(k), C.byref(sp), int(reset)))
        return s.value, k.value, sp.value


class Node:
    """All GPUs of this machine behind the reference's file-level signatures, in one process
    (include/mp3rgain_amd_node.h): one context and one host thread per device, files dealt out by size, the album's
    histogram merged across devices.  `devices` = HIP ordinals, None = every visible device."""

    EXCHANGE_HOST, EXCHANGE_RCCL = 0, 1

    def __init__(self, devices: Optional[Sequence[int]] = None, _backend=None):
        self._lib = _capi.load()
        self._node = None
        if _backend is not None:  # tests: a table of per-device functions instead of rg_ctx
            devs = (C.c_int * len(devices))(*devices)
            self._backend = _backend
            self._node = self._lib.rg_node_create_backend(C.addressof(_backend), devs, len(devices))
        elif devices is None:
            self._node = self._lib.rg_node_create(None, 0)
        else:
            devs = (C.c_int * max(1, len(devices)))(*devices)
            self._node = self._lib.rg_node_create(devs, len(devices))
        if not self._node:
            raise ReplayGainError(-4, self._lib.rg_node_last_error(None).decode("utf-8", "replace"))

    def close(self):
        if self._node:
            self._lib.rg_node_destroy(self._node)
            self._node = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise ReplayGainError(rc, self._lib.rg_node_last_error(self._node).decode("utf-8", "replace"))

    @property
    def devices(self) -> int:
        return int(self._lib.rg_node_devices(self._node))

    def set_exchange(self, mode: int):
        self._check(self._lib.rg_node_set_exchange(self._node, int(mode)))

    def analyzer(self, i: int) -> "Analyzer":
        """The i-th device's context as an Analyzer, for the PCM-level and asynchronous entry points (bench.py's one-process
        mode drives one from a host thread per device).  Owned by the node: closing it releases nothing."""
        ctx = self._lib.rg_node_ctx(self._node, int(i))
        if not ctx:
            raise ReplayGainError(-1, f"node has no context {i}")
        a = Analyzer.__new__(Analyzer)
        a._lib = self._lib
        a._ctx = ctx
        a._borrowed = True
        a.device = int(i)
        a._r128_layout = getattr(self, "_r128_layout", False)
        return a

    def set_tuning(self, key: int, value: int):
        """rg_set_tuning on every device's context."""
        for i in range(self.devices):
            ctx = self._lib.rg_node_ctx(self._node, i)
            if ctx and self._lib.rg_set_tuning(ctx, int(key), int(value)) != 0:
                raise ReplayGainError(-1, self._lib.rg_last_error(ctx).decode("utf-8", "replace"))

    def set_channel_mode_r128(self, mode):
        """Analyzer.set_channel_mode_r128 on every device's context."""
        for i in range(self.devices):
            ctx = self._lib.rg_node_ctx(self._node, i)
            if ctx and self._lib.rg_r128_set_channel_mode(ctx, _r128_mode(mode)) != 0:
                raise ReplayGainError(-1, self._lib.rg_last_error(ctx).decode("utf-8", "replace"))
        self._r128_layout = _r128_mode(mode) == _capi.R128_CHANNELS_LAYOUT

    def set_decoder_command(self, command_template: Optional[str]):
        for i in range(self.devices):
            ctx = self._lib.rg_node_ctx(self._node, i)
            if ctx:
                self._lib.rg_set_decoder_command(ctx, command_template.encode() if command_template else None)

    def analyze_album_files(self, files, track_index: Optional[int] = None) -> AlbumGainResult:
        """analyze_album_with_index (src/replaygain.rs:1044-1074) over all devices."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.TrackResult * max(1, n))()
        alb = _capi.AlbumResult()
        self._check(self._lib.rg_analyze_album_node(self._node, paths, n, -1 if track_index is None else int(track_index), out, C.byref(alb)))
        return AlbumGainResult([_to_result(out[i], out[i].file_type) for i in range(n)], alb.album_loudness_db,
                               alb.album_gain_db, alb.album_peak)

    def analyze_albums_files(self, albums, track_index: Optional[int] = None) -> list:
        """Analyzer.analyze_albums_files over all devices: whole albums dealt out by their files' bytes, one call per device."""
        args = _albums_args(albums, track_index)
        self._check(self._lib.rg_analyze_albums_node(self._node, *args[:-1]))
        return _albums_results(args, lambda i: self._lib.rg_node_tracks_error(self._node, i))

    def analyze_track_files(self, files, track_index: Optional[int] = None) -> list:
        """analyze_track for every file (`-r`), the files dealt out over all devices; per file a result or its error."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.TrackResult * max(1, n))()
        status = (C.c_int32 * max(1, n))()
        self._check(self._lib.rg_analyze_tracks_node(self._node, paths, n, -1 if track_index is None else int(track_index), out, status))
        res = []
        for i in range(n):
            if status[i] == 0:
                res.append(_to_result(out[i], out[i].file_type))
            else:
                res.append(ReplayGainError(int(status[i]), self._lib.rg_node_tracks_error(self._node, i).decode("utf-8", "replace")))
        return res

    def analyze_albums_files_r128(self, albums, true_peak: bool = False, track_index: Optional[int] = None,
                                  dynamics: bool = False) -> list:
        """Analyzer.analyze_albums_files_r128 over all devices: whole albums dealt out by their files' bytes, one call per device."""
        args = _albums_args_r128(albums, track_index, true_peak, dynamics)
        rest = args[:-1] if dynamics else args[:-1] + (None, None)
        self._check(self._lib.rg_r128_analyze_albums_node(self._node, *rest))
        return _albums_results_r128(args, lambda i: self._lib.rg_node_tracks_error(self._node, i))

    def analyze_track_files_r128(self, files, true_peak: bool = False, track_index: Optional[int] = None, dynamics: bool = False) -> list:
        """Analyzer.analyze_track_files_r128, the files dealt out over all devices; per file a result or its error."""
        n = len(files)
        paths = (C.c_char_p * max(1, n))(*[os.fsencode(os.fspath(f)) for f in files])
        out = (_capi.R128TrackResult * max(1, n))()
        status = (C.c_int32 * max(1, n))()
        dyn = (_capi.R128Dynamics * max(1, n))() if dynamics else None
        self._check(self._lib.rg_r128_analyze_tracks_node(self._node, paths, n, -1 if track_index is None else int(track_index),
                                                          int(true_peak), out, status, dyn))
        return [_to_r128(out[i], AudioFileType.Mp3, dyn[i] if dyn is not None else None) if status[i] == 0 else
                ReplayGainError(int(status[i]), self._lib.rg_node_tracks_error(self._node, i).decode("utf-8", "replace")) for i in range(n)]

    def analyze_track_file(self, file_path, track_index: Optional[int] = None) -> ReplayGainResult:
        """analyze_track_with_index (src/replaygain.rs:935-941) on the node's first device."""
        ctx = self._lib.rg_node_ctx(self._node, 0)
        if not ctx:
            r = self.analyze_track_files([file_path], track_index)[0]
            if isinstance(r, ReplayGainError):
                raise r
            return r
        out = _capi.TrackResult()
        rc = self._lib.rg_analyze_track(ctx, os.fsencode(os.fspath(file_path)), -1 if track_index is None else int(track_index), C.byref(out))
        if rc != 0:
            raise ReplayGainError(rc, self._lib.rg_last_error(ctx).decode("utf-8", "replace"))
        return _to_result(out, out.file_type)

    def find_peak_amplitude_file(self, file_path) -> PeakAmplitudeResult:
        """find_peak_amplitude (src/replaygain.rs:1140-1249) on the node's first device."""
        ctx = self._lib.rg_node_ctx(self._node, 0)
        pk = _capi.PeakResult()
        rc = self._lib.rg_find_peak_amplitude(ctx, os.fsencode(os.fspath(file_path)), C.byref(pk))
        if rc != 0:
            raise ReplayGainError(rc, self._lib.rg_last_error(ctx).decode("utf-8", "replace"))
        return PeakAmplitudeResult(pk.peak, pk.peak_pcm, pk.sample_rate)

    def last_partition(self, n: int) -> List[int]:
        own = (C.c_uint32 * max(1, n))()
        self._check(self._lib.rg_node_last_partition(self._node, own, n))
        return [int(own[i]) for i in range(n)]


def node_partition(sizes: Sequence[int], world: int) -> List[int]:
    """rg_node_partition: device of every item (heaviest first, each to the least loaded device)."""
    lib = _capi.load()
    n = len(sizes)
    a = (C.c_uint64 * max(1, n))(*[int(x) for x in sizes])
    own = (C.c_uint32 * max(1, n))()
    lib.rg_node_partition(a, n, world, own)
    return [int(own[i]) for i in range(n)]


def _albums_args(albums, track_index: Optional[int]):
    """rg_analyze_albums' arguments after the context / node, plus the album sizes."""
    sizes = [len(a) for a in albums]
    files = [os.fsencode(os.fspath(f)) for a in albums for f in a]
    n, n_albums = len(files), len(sizes)
    first = [0]
    for k in sizes:
        first.append(first[-1] + k)
    paths = (C.c_char_p * max(1, n))(*files)
    album_first = (C.c_size_t * (n_albums + 1))(*first)
    out = (_capi.TrackResult * max(1, n))()
    status = (C.c_int32 * max(1, n))()
    alb = (_capi.AlbumResult * max(1, n_albums))()
    alb_status = (C.c_int32 * max(1, n_albums))()
    return (paths, n, album_first, n_albums, -1 if track_index is None else int(track_index), out, status, alb, alb_status, first)


def _albums_results(args, file_error) -> list:
    _, _, _, n_albums, _, out, status, alb, alb_status, first = args
    res = []
    for a in range(n_albums):
        files = range(first[a], first[a + 1])
        if alb_status[a] != 0:
            bad = next((i for i in files if status[i] != 0), None)
            text = file_error(bad).decode("utf-8", "replace") if bad is not None else ""
            res.append(ReplayGainError(int(alb_status[a]), text))
            continue
        res.append(AlbumGainResult([_to_result(out[i], out[i].file_type) for i in files], alb[a].album_loudness_db,
                                   alb[a].album_gain_db, alb[a].album_peak))
    return res


def _albums_args_r128(albums, track_index: Optional[int], true_peak: bool, dynamics: bool):
    """rg_r128_analyze_albums[_dynamics]' arguments after the context / node, plus the album sizes."""
    paths, n, album_first, n_albums, ti, _, status, _, alb_status, first = _albums_args(albums, track_index)
    out = (_capi.R128TrackResult * max(1, n))()
    alb = (_capi.R128AlbumResult * max(1, n_albums))()
    args = (paths, n, album_first, n_albums, ti, int(true_peak), out, status, alb, alb_status)
    if dynamics:
        args += ((_capi.R128Dynamics * max(1, n))(), (_capi.R128Dynamics * max(1, n_albums))())
    return args + (first,)


def _albums_results_r128(args, file_error) -> list:
    n_albums, out, status, alb, alb_status, first = args[3], args[6], args[7], args[8], args[9], args[-1]
    dyn, adyn = (args[10], args[11]) if len(args) == 13 else (None, None)
    res = []
    for a in range(n_albums):
        files = range(first[a], first[a + 1])
        if alb_status[a] != 0:
            bad = next((i for i in files if status[i] != 0), None)
            text = file_error(bad).decode("utf-8", "replace") if bad is not None else ""
            res.append(ReplayGainError(int(alb_status[a]), text))
            continue
        res.append(_to_r128_album([_to_r128(out[i], AudioFileType.Mp3, dyn[i] if dyn is not None else None) for i in files], alb[a],
                                  adyn[a] if adyn is not None else None))
    return res


def _to_result(r: _capi.TrackResult, file_type: AudioFileType) -> ReplayGainResult:
    return ReplayGainResult(r.loudness_db, r.gain_db, r.peak, r.sample_rate, AudioFileType(int(file_type)), r.windows, r.flags)


_default: Optional[Analyzer] = None


def _default_analyzer() -> Analyzer:
    global _default
    if _default is None:
        _default = Analyzer(0)
    return _default


def _is_path(x) -> bool:
    return isinstance(x, (str, bytes, os.PathLike))


def analyze_track(track) -> ReplayGainResult:
    """analyze_track (src/replaygain.rs:929-932) for a file path, or for decoded PCM (PcmTrack)."""
    a = _default_analyzer()
    return a.analyze_track_file(track) if _is_path(track) else a.analyze_track(track)


def analyze_track_with_index(file_path, track_index: Optional[int]) -> ReplayGainResult:
    return _default_analyzer().analyze_track_file(file_path, track_index)


def analyze_album(tracks) -> AlbumGainResult:
    """analyze_album (src/replaygain.rs:1033-1036) for file paths, or for decoded PCM (PcmTracks)."""
    a = _default_analyzer()
    tracks = list(tracks)
    return a.analyze_album_files(tracks) if tracks and _is_path(tracks[0]) else a.analyze_album(tracks)


def analyze_album_with_index(files, track_index: Optional[int]) -> AlbumGainResult:
    return _default_analyzer().analyze_album_files(list(files), track_index)


def find_peak_amplitude(track) -> PeakAmplitudeResult:
    a = _default_analyzer()
    return a.find_peak_amplitude_file(track) if _is_path(track) else a.find_peak_amplitude(track)


def set_decoder_command(command_template: Optional[str]) -> None:
    _default_analyzer().set_decoder_command(command_template)
