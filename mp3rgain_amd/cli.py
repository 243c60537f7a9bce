"""Command-line façade: mp3rgain's option set and output lines over this
library -- `python -m mp3rgain_amd [OPTIONS] <FILES>...`.

Behaviour follows mp3rgain v1.5.0 src/main.rs (function by function, cited below); colours and the progress
bar are left out (the reference drops both when stdout is not a terminal).  ReplayGain analysis (-r, -a, -e,
-x, TSV info) runs on the GPU through the C ABI; it needs decoded audio, so an analysed file is a WAV file, or
any file when a decoder command is given (`--decoder "ffmpeg -v error -i {} -f wav -c:a pcm_f32le -"` or the
MP3RGAIN_AMD_DECODER environment variable).  Gain changes, undo and tags are the lossless byte work of
`mp3gain` / `mp4meta` and need no decoder.
"""
from __future__ import annotations

import json
import math
import os
import shutil
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Tuple

from . import _capi, mp3gain, mp4meta
from . import replaygain as rgmod

VERSION = "0.1.0"
GAIN_STEP_DB = 1.5
REFERENCE_DB = 89.0


class CliError(Exception):
    """An anyhow error that leaves main(): printed as `Error: ...`, exit status 1."""


class Exit(Exception):
    def __init__(self, code: int):
        self.code = code


@dataclass
class Options:  # src/main.rs:65-96
    gain_steps: Optional[int] = None
    gain_modifier_db: float = 0.0
    channel_gain: Optional[Tuple[int, int]] = None
    gain_modifier: int = 0
    undo: bool = False
    stored_tag_mode: str = "none"  # none | check | delete | skip | recalc | id3v2 | apev2
    track_gain: bool = False
    album_gain: bool = False
    skip_album: bool = False
    max_amplitude_only: bool = False
    track_index: Optional[int] = None
    preserve_timestamp: bool = False
    ignore_clipping: bool = False
    prevent_clipping: bool = False
    quiet: bool = False
    recursive: bool = False
    dry_run: bool = False
    output_format: str = "text"  # text | json | tsv
    wrap_gain: bool = False
    use_temp_file: bool = False
    assume_mpeg2: bool = False
    decoder: Optional[str] = None  # this façade only
    r128: bool = False       # this façade only: EBU R 128 / ReplayGain 2.0 analysis instead of ReplayGain 1.0
    true_peak: bool = False  # with --r128: report and clip-limit on the true peak
    loudness_range: bool = False  # with --r128 (--range): loudness range, maximum momentary and short-term loudness
    surround: bool = False   # with --r128 (--surround): BS.1770 channel weights from every file's channel layout
    verify: bool = False     # this façade only (--verify): FLAC files against the MD5 signature of their STREAMINFO
    rip: bool = False        # this façade only (--rip): the files are the tracks of one disc; CRC-32 and AccurateRip checksums
    rip_log: Optional[str] = None  # with --rip (--rip-log LOG): a ripper's log to compare the checksums with
    rip_offsets: bool = False  # with --rip --rip-log (--rip-offsets): look for the log's drive offset within +-2939 samples
    stats: bool = False      # this façade only (--stats): clipping runs, dropouts, DC offset, padded bits, edge silence per file
    clip_run: Optional[int] = None  # with --stats (--clip-run N): full-scale samples in a row that count as a clip run
    zero_run: Optional[int] = None  # with --stats (--zero-run N): zero samples in a row inside the audio that count as a dropout
    spectrum: bool = False   # this façade only (--spectrum): where the spectrum ends, per file and channel (lossy transcodes, upsampled files)
    edge_db: Optional[float] = None  # with --spectrum (--edge-db DB): how far the spectrum must fall across the edge
    min_cutoff: Optional[float] = None  # with --spectrum (--min-cutoff HZ): edges below this frequency are not reported
    dr: bool = False         # this façade only (--dr): the dynamic range (DR) figure per file, and the album's
    dr_top: Optional[int] = None  # with --dr (--dr-top PERMILLE): the share of the loudest blocks that count, in per mille
    ancestry: bool = False   # this façade only (--ancestry): is this PCM a decoded MP3?  The granule grid, per file and view
    ancestry_segments: Optional[int] = None  # with --ancestry (--ancestry-segments S): segments per file, 0 = the whole file
    ancestry_granules: Optional[int] = None  # with --ancestry (--ancestry-granules G): granules per segment
    duplicates: bool = False  # this façade only (--duplicates): which of these files are the same recording?  Fingerprints and every pair
    dup_radius: Optional[float] = None  # with --duplicates (--dup-radius SECONDS): the largest offset looked for, in seconds at 44.1 kHz
    dup_any_rate: bool = False  # with --duplicates (--dup-any-rate): every file brought to 11025 Hz first, so copies at different sample rates match
    dup_ber: Optional[int] = None  # with --duplicates (--dup-ber PERMILLE): the share of differing bits up to which a pair matches
    tempo: bool = False  # this façade only (--tempo): how fast is each file?  BPM and a constant-tempo beat grid
    tempo_min: Optional[int] = None  # with --tempo (--tempo-min BPM): the reading lies in [BPM, 2 BPM)
    key: bool = False  # this façade only (--key): in which musical key is each file?  One of 12 major and 12 minor keys
    key_segment: Optional[int] = None  # with --key (--key-segment ROWS): the rows of a segment of the steadiness figure
    stereo: bool = False  # this façade only (--stereo): how do the two channels of each file relate?  Dual mono, inverted, delayed, ...
    encode: bool = False  # this façade only (--encode): WAV and FLAC files to FLAC, encoded on the GPU, verified before they are written
    encode_dir: Optional[Path] = None  # with --encode (--encode-dir DIR, required): where <stem>.flac goes
    encode_lpc: Optional[int] = None  # with --encode (--encode-lpc N): the largest LPC order tried
    encode_block: Optional[int] = None  # with --encode (--encode-block N): the block size
    encode_verify: bool = True  # --no-encode-verify clears it
    compare: bool = False  # this façade only (--compare REF FILE...): a null test of every file against the first
    compare_radius: Optional[int] = None  # with --compare (--compare-radius N): how far from the hint the fine lag is looked for, in samples
    compare_hint: Optional[int] = None  # with --compare (--compare-hint FRAMES): the expected lag of every file, instead of the fingerprint match
    stereo_radius: Optional[int] = None  # with --stereo (--stereo-radius N): the largest channel delay looked for, in samples
    clicks: bool = False  # this façade only (--clicks): are there clicks or glitches in each file?  Residual of a linear predictor against its local median
    click_ratio: Optional[float] = None  # with --clicks (--click-ratio X): a sample is flagged when its residual is more than X times the scale
    click_order: Optional[int] = None  # with --clicks (--click-order P): the predictor's order
    click_block: Optional[int] = None  # with --clicks (--click-block B): the samples of a block
    click_list: Optional[int] = None  # with --clicks (--click-list K): how many events are listed per file
    files: List[Path] = field(default_factory=list)


def _rust_float(x: float) -> str:
    """`{}` of an f64: 89.0 -> "89", 1.5 -> "1.5"."""
    return str(int(x)) if x == int(x) and abs(x) < 1e15 else repr(x)


def _parse_int(s: str, what: str, bits: int = 32, signed: bool = True) -> int:
    try:
        if s.strip() != s or s.startswith("+-") or "_" in s:
            raise ValueError
        v = int(s, 10)
    except ValueError:
        raise CliError(f"{what}: {s}")
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    if not lo <= v <= hi:
        raise CliError(f"{what}: {s}")
    return v


def _parse_float(s: str, what: str) -> float:
    try:
        if s.strip() != s or "_" in s:
            raise ValueError
        return float(s)
    except ValueError:
        raise CliError(f"{what}: {s}")


def _parse_positive(s: str, what: str) -> float:
    v = _parse_float(s, what)
    if not (v > 0.0 and v != float("inf")):
        raise CliError(f"{what}: {s}")
    return v


def parse_args(args: List[str], out, err) -> Options:
    """parse_args, src/main.rs:183-434."""
    o = Options()
    i = 0

    def need(flag: str, msg: str) -> str:
        nonlocal i
        i += 1
        if i >= len(args):
            print(f"error: {msg}", file=err)
            raise Exit(1)
        return args[i]

    while i < len(args):
        arg = args[i]
        if arg == "--dry-run":
            o.dry_run = True
        elif arg == "--help":
            print_usage(out)
            raise Exit(0)
        elif arg == "--version":
            print_version(out)
            raise Exit(0)
        elif arg == "--r128":  # not in the reference: integrated loudness (BS.1770), gain to -18 LUFS
            o.r128 = True
        elif arg == "--true-peak":
            o.true_peak = True
        elif arg == "--range":
            o.loudness_range = True
        elif arg == "--surround":
            o.surround = True
        elif arg == "--verify":  # not in the reference: a command of its own, like -s c
            o.verify = True
        elif arg == "--rip":  # not in the reference: a command of its own, like --verify
            o.rip = True
        elif arg == "--rip-offsets":
            o.rip_offsets = True
        elif arg == "--rip-log":
            o.rip_log = need("--rip-log", "--rip-log requires an argument")
        elif arg == "--stats":  # not in the reference: a command of its own, like --verify and --rip
            o.stats = True
        elif arg == "--clip-run":
            o.clip_run = _parse_int(need("--clip-run", "--clip-run requires an argument"), "invalid run length", 32, signed=False)
        elif arg == "--zero-run":
            o.zero_run = _parse_int(need("--zero-run", "--zero-run requires an argument"), "invalid run length", 32, signed=False)
        elif arg == "--spectrum":  # not in the reference: a command of its own, like --stats
            o.spectrum = True
        elif arg == "--edge-db":
            o.edge_db = _parse_positive(need("--edge-db", "--edge-db requires an argument"), "invalid edge depth")
        elif arg == "--min-cutoff":
            o.min_cutoff = _parse_positive(need("--min-cutoff", "--min-cutoff requires an argument"), "invalid frequency")
        elif arg == "--dr":  # not in the reference: a command of its own, like --stats
            o.dr = True
        elif arg == "--dr-top":
            o.dr_top = _parse_int(need("--dr-top", "--dr-top requires an argument"), "invalid per mille value", 32, signed=False)
        elif arg == "--ancestry":  # not in the reference: a command of its own, like --stats
            o.ancestry = True
        elif arg == "--ancestry-segments":
            o.ancestry_segments = _parse_int(need("--ancestry-segments", "--ancestry-segments requires an argument"), "invalid segment count", 32, signed=False)
        elif arg == "--ancestry-granules":
            o.ancestry_granules = _parse_int(need("--ancestry-granules", "--ancestry-granules requires an argument"), "invalid granule count", 32, signed=False)
        elif arg == "--duplicates":  # not in the reference: a command of its own, like --stats
            o.duplicates = True
        elif arg == "--dup-any-rate":
            o.dup_any_rate = True
        elif arg == "--dup-radius":
            o.dup_radius = _parse_positive(need("--dup-radius", "--dup-radius requires an argument"), "invalid radius")
        elif arg == "--dup-ber":
            o.dup_ber = _parse_int(need("--dup-ber", "--dup-ber requires an argument"), "invalid per mille value", 32, signed=False)
        elif arg == "--tempo":  # not in the reference: a command of its own, like --duplicates
            o.tempo = True
        elif arg == "--tempo-min":
            o.tempo_min = _parse_int(need("--tempo-min", "--tempo-min requires an argument"), "invalid BPM", 32, signed=False)
        elif arg == "--key":  # not in the reference: a command of its own, like --tempo
            o.key = True
        elif arg == "--key-segment":
            o.key_segment = _parse_int(need("--key-segment", "--key-segment requires an argument"), "invalid number of rows", 32, signed=False)
        elif arg == "--stereo":  # not in the reference: a command of its own, like --dr
            o.stereo = True
        elif arg == "--encode":  # not in the reference: a command of its own
            o.encode = True
        elif arg == "--encode-dir":
            o.encode_dir = Path(need("--encode-dir", "--encode-dir requires an argument"))
        elif arg == "--encode-lpc":
            o.encode_lpc = _parse_int(need("--encode-lpc", "--encode-lpc requires an argument"), "invalid LPC order", 32, signed=False)
        elif arg == "--encode-block":
            o.encode_block = _parse_int(need("--encode-block", "--encode-block requires an argument"), "invalid block size", 32, signed=False)
        elif arg == "--no-encode-verify":
            o.encode_verify = False
        elif arg == "--clicks":  # not in the reference: a command of its own, like --dr
            o.clicks = True
        elif arg == "--click-ratio":
            o.click_ratio = _parse_float(need("--click-ratio", "--click-ratio requires an argument"), "invalid ratio")
        elif arg == "--click-order":
            o.click_order = _parse_int(need("--click-order", "--click-order requires an argument"), "invalid order", 32, signed=False)
        elif arg == "--click-block":
            o.click_block = _parse_int(need("--click-block", "--click-block requires an argument"), "invalid block length", 32, signed=False)
        elif arg == "--click-list":
            o.click_list = _parse_int(need("--click-list", "--click-list requires an argument"), "invalid number of events", 32, signed=False)
        elif arg == "--compare":  # not in the reference: a command of its own, like --stereo
            o.compare = True
        elif arg == "--compare-radius":
            o.compare_radius = _parse_int(need("--compare-radius", "--compare-radius requires an argument"), "invalid radius", 32, signed=False)
        elif arg == "--compare-hint":
            o.compare_hint = _parse_int(need("--compare-hint", "--compare-hint requires an argument"), "invalid hint", 64, signed=True)
        elif arg == "--stereo-radius":
            o.stereo_radius = _parse_int(need("--stereo-radius", "--stereo-radius requires an argument"), "invalid radius", 32, signed=False)
        elif arg == "--decoder":  # not in the reference: see the module docstring
            o.decoder = need("--decoder", "--decoder requires an argument")
        elif arg.startswith("-") and len(arg) > 1 and not arg.startswith("--"):
            flag = arg[1:]
            if flag == "g":
                o.gain_steps = _parse_int(need("g", "-g requires an argument"), "invalid gain value")
            elif flag == "d":
                o.gain_modifier_db = _parse_float(need("d", "-d requires an argument"), "invalid dB value")
            elif flag == "m":
                o.gain_modifier = _parse_int(need("m", "-m requires an argument"), "invalid modifier value")
            elif flag == "s":
                mode = need("s", "-s requires an argument")
                table = {"c": "check", "d": "delete", "s": "skip", "r": "recalc", "i": "id3v2", "a": "apev2"}
                if mode not in table:
                    print(f"error: unknown -s mode '{mode}', use c/d/s/r/i/a", file=err)
                    raise Exit(1)
                o.stored_tag_mode = table[mode]
                if mode == "i":
                    print("warning: -s i (ID3v2 tags) not fully supported, using APEv2", file=err)
            elif flag == "o":
                # mp3gain compatibility: a bare -o means TSV
                if i + 1 < len(args) and args[i + 1].lower() in ("json", "text", "tsv", "db"):
                    i += 1
                    o.output_format = {"json": "json", "text": "text", "tsv": "tsv", "db": "tsv"}[args[i].lower()]
                else:
                    o.output_format = "tsv"
            elif flag == "l":
                two = "-l requires two arguments: <channel> <gain>"
                a = need("l", two)
                try:
                    ch = _parse_int(a, "", 64, signed=False)
                except CliError:
                    raise CliError(f"invalid channel number: {a} (use 0 for left, 1 for right)")
                if ch not in (0, 1):
                    raise CliError(f"invalid channel: {ch} (use 0 for left, 1 for right)")
                o.channel_gain = (ch, _parse_int(need("l", two), "invalid gain value"))
            elif flag == "r":
                o.track_gain = True
            elif flag == "a":
                o.album_gain = True
            elif flag == "e":
                o.skip_album = True
            elif flag == "x":
                o.max_amplitude_only = True
            elif flag == "i":
                o.track_index = _parse_int(need("i", "-i requires an argument"), "invalid track index", 32, signed=False)
            elif flag == "u":
                o.undo = True
            elif flag == "p":
                o.preserve_timestamp = True
            elif flag == "c":
                o.ignore_clipping = True
            elif flag == "k":
                o.prevent_clipping = True
            elif flag == "q":
                o.quiet = True
            elif flag == "R":
                o.recursive = True
            elif flag == "n":
                o.dry_run = True
            elif flag == "w":
                o.wrap_gain = True
            elif flag == "t":
                o.use_temp_file = True
            elif flag == "f":
                o.assume_mpeg2 = True
            elif flag in ("v", "-version"):
                print_version(out)
                raise Exit(0)
            elif flag in ("h", "-help"):
                print_usage(out)
                raise Exit(0)
            elif all(c in "pqckuranRewxtf" for c in flag):  # combined short flags: -qp, -kc ...
                names = {"p": "preserve_timestamp", "q": "quiet", "c": "ignore_clipping", "k": "prevent_clipping",
                         "u": "undo", "r": "track_gain", "a": "album_gain", "n": "dry_run", "R": "recursive",
                         "e": "skip_album", "w": "wrap_gain", "x": "max_amplitude_only", "t": "use_temp_file",
                         "f": "assume_mpeg2"}
                for c in flag:
                    setattr(o, names[c], True)
            elif flag.startswith("g"):  # attached values: -g2, -d4.5, -m2, -i1
                o.gain_steps = _parse_int(flag[1:], "invalid gain value")
            elif flag.startswith("d"):
                o.gain_modifier_db = _parse_float(flag[1:], "invalid dB value")
            elif flag.startswith("m"):
                o.gain_modifier = _parse_int(flag[1:], "invalid modifier value")
            elif flag.startswith("i"):
                o.track_index = _parse_int(flag[1:], "invalid track index", 32, signed=False)
            else:
                print(f"warning: unknown option: -{flag}", file=err)
        elif not arg.startswith("--"):
            o.files.append(Path(arg))
        i += 1
    if o.surround and not o.r128:
        raise CliError("--surround requires --r128")
    if o.rip_log is not None and not o.rip:
        raise CliError("--rip-log requires --rip")
    if o.rip_offsets and not o.rip:
        raise CliError("--rip-offsets requires --rip")
    if o.rip_offsets and o.rip_log is None:
        raise CliError("--rip-offsets requires --rip-log")
    if o.clip_run is not None and not o.stats:
        raise CliError("--clip-run requires --stats")
    if o.zero_run is not None and not o.stats:
        raise CliError("--zero-run requires --stats")
    if o.clip_run == 0 or o.zero_run == 0:
        raise CliError("--clip-run and --zero-run take a length of at least 1")
    if o.edge_db is not None and not o.spectrum:
        raise CliError("--edge-db requires --spectrum")
    if o.min_cutoff is not None and not o.spectrum:
        raise CliError("--min-cutoff requires --spectrum")
    if o.dr_top is not None and not o.dr:
        raise CliError("--dr-top requires --dr")
    if o.dr_top is not None and not 1 <= o.dr_top <= 1000:
        raise CliError(f"--dr-top takes 1 to 1000 per mille: {o.dr_top}")
    if o.dr:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--r128", o.r128),
                                        ("-x", o.max_amplitude_only), ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo),
                                        ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--dr is a command of its own and cannot be combined with {', '.join(others)}")
    if o.ancestry_segments is not None and not o.ancestry:
        raise CliError("--ancestry-segments requires --ancestry")
    if o.ancestry_granules is not None and not o.ancestry:
        raise CliError("--ancestry-granules requires --ancestry")
    if o.ancestry_granules == 0:
        raise CliError("--ancestry-granules takes at least 1")
    if o.ancestry:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--r128", o.r128), ("-x", o.max_amplitude_only), ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo),
                                        ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--ancestry is a command of its own and cannot be combined with {', '.join(others)}")
    if o.dup_radius is not None and not o.duplicates:
        raise CliError("--dup-radius requires --duplicates")
    if o.dup_ber is not None and not o.duplicates:
        raise CliError("--dup-ber requires --duplicates")
    if o.dup_any_rate and not o.duplicates:
        raise CliError("--dup-any-rate requires --duplicates")
    if o.dup_ber is not None and not 1 <= o.dup_ber <= 1000:
        raise CliError(f"--dup-ber takes 1 to 1000 per mille: {o.dup_ber}")
    if o.dup_radius is not None and o.dup_any_rate and not 1 <= dup_radius_codes(o.dup_radius, _capi.RS_RATE_OUT) <= _capi.FP_MAX_RADIUS:
        raise CliError(f"--dup-radius takes {512 / _capi.RS_RATE_OUT:.3f} to {_capi.FP_MAX_RADIUS * 512 / _capi.RS_RATE_OUT:.1f} seconds with --dup-any-rate: "
                       f"{o.dup_radius}")
    if o.dup_radius is not None and not o.dup_any_rate and not 1 <= dup_radius_codes(o.dup_radius) <= _capi.FP_MAX_RADIUS:
        raise CliError(f"--dup-radius takes {512 / 44100:.3f} to {_capi.FP_MAX_RADIUS * 512 / 44100:.1f} seconds: {o.dup_radius}")
    if o.duplicates:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--r128", o.r128), ("-x", o.max_amplitude_only), ("-r", o.track_gain),
                                        ("-a", o.album_gain), ("-u", o.undo), ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--duplicates is a command of its own and cannot be combined with {', '.join(others)}")
    if o.tempo_min is not None and not o.tempo:
        raise CliError("--tempo-min requires --tempo")
    if o.tempo_min is not None and not 30 <= o.tempo_min <= 300:
        raise CliError(f"--tempo-min takes 30 to 300 BPM: {o.tempo_min}")
    if o.tempo:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--r128", o.r128), ("-x", o.max_amplitude_only),
                                        ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo), ("-g", o.gain_steps is not None),
                                        ("-l", o.channel_gain is not None), ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--tempo is a command of its own and cannot be combined with {', '.join(others)}")
    if o.key_segment is not None and not o.key:
        raise CliError("--key-segment requires --key")
    if o.key_segment is not None and not 8 <= o.key_segment <= 4096:
        raise CliError(f"--key-segment takes 8 to 4096 rows: {o.key_segment}")
    if o.key:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--tempo", o.tempo), ("--r128", o.r128),
                                        ("-x", o.max_amplitude_only), ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo),
                                        ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--key is a command of its own and cannot be combined with {', '.join(others)}")
    if o.stereo_radius is not None and not o.stereo:
        raise CliError("--stereo-radius requires --stereo")
    if o.stereo_radius is not None and not 0 <= o.stereo_radius <= _capi.ST_MAX_RADIUS:
        raise CliError(f"--stereo-radius takes 0 to {_capi.ST_MAX_RADIUS} samples: {o.stereo_radius}")
    if o.stereo:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--tempo", o.tempo), ("--key", o.key),
                                        ("--r128", o.r128), ("-x", o.max_amplitude_only), ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo),
                                        ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--stereo is a command of its own and cannot be combined with {', '.join(others)}")
    for name, v in (("--compare-radius", o.compare_radius), ("--compare-hint", o.compare_hint)):
        if v is not None and not o.compare:
            raise CliError(f"{name} requires --compare")
    if o.compare_radius is not None and not 0 <= o.compare_radius <= _capi.CMP_MAX_RADIUS:
        raise CliError(f"--compare-radius takes 0 to {_capi.CMP_MAX_RADIUS} samples: {o.compare_radius}")
    if o.compare_hint is not None and abs(o.compare_hint) > _capi.CMP_MAX_HINT:
        raise CliError(f"--compare-hint takes at most 2^32 frames either way: {o.compare_hint}")
    if o.compare:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--tempo", o.tempo), ("--key", o.key),
                                        ("--stereo", o.stereo), ("--clicks", o.clicks), ("--encode", o.encode), ("--r128", o.r128),
                                        ("-x", o.max_amplitude_only), ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo),
                                        ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--compare is a command of its own and cannot be combined with {', '.join(others)}")
        if len(o.files) < 2:
            raise CliError("--compare takes the reference copy and at least one file to hold against it")
    given = [name for name, on in (("--click-ratio", o.click_ratio is not None), ("--click-order", o.click_order is not None),
                                   ("--click-block", o.click_block is not None), ("--click-list", o.click_list is not None)) if on]
    if given and not o.clicks:
        raise CliError(f"{given[0]} requires --clicks")
    if o.click_ratio is not None and not (math.isfinite(o.click_ratio) and 1.0 <= o.click_ratio <= 1000.0):
        raise CliError(f"--click-ratio takes 1 to 1000 times the scale: {o.click_ratio}")
    if o.click_order is not None and (o.click_order % 2 or not 2 <= o.click_order <= _capi.CK_MAX_ORDER):
        raise CliError(f"--click-order takes an even order from 2 to {_capi.CK_MAX_ORDER}: {o.click_order}")
    if o.click_block is not None and o.click_block not in (256, 512, 1024, 2048, 4096):
        raise CliError(f"--click-block takes 256, 512, 1024, 2048 or 4096: {o.click_block}")
    if o.click_list is not None and not 0 <= o.click_list <= _capi.CK_MAX_EVENTS:
        raise CliError(f"--click-list takes 0 to {_capi.CK_MAX_EVENTS} events: {o.click_list}")
    if o.clicks:
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--tempo", o.tempo), ("--key", o.key),
                                        ("--stereo", o.stereo), ("--encode", o.encode), ("--r128", o.r128), ("-x", o.max_amplitude_only),
                                        ("-r", o.track_gain), ("-a", o.album_gain), ("-u", o.undo), ("-g", o.gain_steps is not None),
                                        ("-l", o.channel_gain is not None), ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--clicks is a command of its own and cannot be combined with {', '.join(others)}")
    if not o.encode:
        given = [name for name, on in (("--encode-dir", o.encode_dir is not None), ("--encode-lpc", o.encode_lpc is not None),
                                       ("--encode-block", o.encode_block is not None), ("--no-encode-verify", not o.encode_verify)) if on]
        if given:
            raise CliError(f"{given[0]} requires --encode")
    else:
        if o.encode_dir is None:
            raise CliError("--encode requires --encode-dir DIR")
        if o.encode_lpc is not None and not 0 <= o.encode_lpc <= _capi.FLAC_ENC_MAX_LPC:
            raise CliError(f"--encode-lpc takes 0 to {_capi.FLAC_ENC_MAX_LPC}: {o.encode_lpc}")
        if o.encode_block is not None and o.encode_block not in (256, 512, 1024, 2048, 4096):
            raise CliError(f"--encode-block takes 256, 512, 1024, 2048 or 4096: {o.encode_block}")
        others = [name for name, on in (("--verify", o.verify), ("--rip", o.rip), ("--stats", o.stats), ("--spectrum", o.spectrum), ("--dr", o.dr),
                                        ("--ancestry", o.ancestry), ("--duplicates", o.duplicates), ("--tempo", o.tempo), ("--key", o.key),
                                        ("--stereo", o.stereo), ("--r128", o.r128), ("-x", o.max_amplitude_only), ("-r", o.track_gain),
                                        ("-a", o.album_gain), ("-u", o.undo), ("-g", o.gain_steps is not None), ("-l", o.channel_gain is not None),
                                        ("-s", o.stored_tag_mode in ("check", "delete"))) if on]
        if others:
            raise CliError(f"--encode is a command of its own and cannot be combined with {', '.join(others)}")
    return o


def _click_time(sample: int, rate: int) -> str:
    """A sample's place as m:ss.mmm."""
    ms = (sample * 1000) // rate if rate else 0
    return f"{ms // 60000}:{ms // 1000 % 60:02d}.{ms % 1000:03d}"


def _click_channel(c: int, channels: int) -> str:
    """A channel as the text names it: nothing for a mono file, left and right for two channels, `ch N` beyond."""
    return "" if channels == 1 else (" left", " right")[c] if channels == 2 else f" ch {c}"


def clicks_line(r) -> str:
    """A file's reading as the text output has it (without the name): `no clicks`, or `3 clicks (first at 1:02.345 left, strongest
    x41.2 at 2:10.007 right)`, and the bursts behind it."""
    n, b = r.clicks, r.bursts
    line = "no clicks"
    if n:
        at, c = r.first_click
        s, s_at, s_c = r.strongest_click
        line = (f"{n} click{'s' if n != 1 else ''} (first at {_click_time(at, r.sample_rate)}{_click_channel(c, r.channels)}, "
                f"strongest x{s / 1000.0:.1f} at {_click_time(s_at, r.sample_rate)}{_click_channel(s_c, r.channels)})")
    return line + (f", {b} burst{'s' if b != 1 else ''}" if b else "")


def click_event_line(e, r) -> str:
    """One listed event as the text output has it."""
    return f"    {e.kind} at {_click_time(e.start, r.sample_rate)}{_click_channel(e.channel, r.channels)}, {e.width} sample{'s' if e.width != 1 else ''}, x{e.strength_permille / 1000.0:.1f}"


def _signed_db(x: float) -> str:
    return f"{x:+.1f} dB" if math.isfinite(x) else ("+inf dB" if x > 0 else "-inf dB")


def stereo_line(r) -> str:
    """A file's reading as the text output has it (without the name): the first verdict that names what the file is, then the
    figures."""
    v = r.verdicts
    if "mono file" in v:
        return "mono file"
    if "silent" in v:
        return "silent"
    if "dual mono" in v:
        return "dual mono"
    if "inverted copy" in v:
        return "right channel is the inverted left"
    figures = f"correlation {r.correlation:.2f}, side {_signed_db(r.side_db)}, balance {_signed_db(r.balance_db)}"
    if "delayed" in v:
        who = "right" if r.lag > 0 else "left"
        return f"{who} channel late by {abs(r.lag)} sample{'s' if abs(r.lag) != 1 else ''} (correlation {r.lag_correlation:.3f} there, {r.correlation:.2f} in place)"
    if "out of phase" in v:
        return f"channels out of phase  ({figures})"
    if "one-sided" in v:
        return f"one-sided  ({figures})"
    if "near mono" in v:
        return f"near mono  ({figures})"
    return f"stereo  ({figures})"


def key_line(r) -> str:
    """A file's reading as the text output has it (without the name)."""
    if not r.found:
        return "no key found"
    return f"{r.name}  ({r.camelot}, correlation {r.correlation:.2f}, margin {r.margin:.2f}, steady {r.steady:.2f})"


def tempo_line(r) -> str:
    """A file's reading as the text output has it (without the name)."""
    if not r.found:
        return "no tempo found"
    return f"{r.bpm:.2f} BPM  (confidence {r.confidence:.2f}, steady {r.steady:.2f}, first beat {r.first_beat_seconds:.3f} s)"


def dup_radius_codes(seconds: float, rate: float = 44100.0) -> int:
    """--dup-radius in codes of 512 samples, taken at 44.1 kHz (with --dup-any-rate: at the common rate, 11025 Hz)."""
    return int(round(seconds * rate / 512.0))


# ---- JSON shapes (src/main.rs:101-165): field order of the structs, None fields skipped -----------------------
_FILE_KEYS = ("file", "status", "frames", "mpeg_version", "channel_mode", "min_gain", "max_gain", "avg_gain",
              "headroom_steps", "headroom_db", "gain_applied_steps", "gain_applied_db", "loudness_db", "loudness_lufs",
              "loudness_range_lu", "max_momentary_lufs", "max_short_term_lufs", "peak",
              "max_amplitude", "error", "warning", "dry_run")


def _is_riff_wave(file) -> bool:
    try:
        with open(file, "rb") as f:
            head = f.read(12)
    except OSError:
        return False
    return len(head) == 12 and head[:4] == b"RIFF" and head[8:] == b"WAVE"


def _is_flac(file) -> bool:
    """A native FLAC stream by its bytes ("fLaC", also behind an ID3v2 tag), as _is_riff_wave recognises WAV."""
    try:
        with open(file, "rb") as f:
            head = f.read(10)
            skip = 0
            if len(head) == 10 and head[:3] == b"ID3" and not any(b & 0x80 for b in head[6:10]):
                skip = 10 + ((head[6] << 21) | (head[7] << 14) | (head[8] << 7) | head[9]) + (10 if head[5] & 0x10 else 0)
            f.seek(skip)
            return f.read(4) == b"fLaC"
    except OSError:
        return False


def _lufs(rg):
    """loudness_lufs of a result of the --r128 analysis, None (no JSON field) otherwise."""
    return getattr(rg, "loudness_lufs", None)


def _dyn(rg) -> dict:
    """The JSON fields of --range (loudness_range_lu, max_momentary_lufs, max_short_term_lufs) of a result of the --r128
    analysis that carries them, nothing otherwise."""
    d = getattr(rg, "dynamics", None)
    if d is None:
        return {}
    return {"loudness_range_lu": d.loudness_range_lu, "max_momentary_lufs": d.max_momentary_lufs,
            "max_short_term_lufs": d.max_short_term_lufs}


def _dyn_text(d) -> str:
    return (f"Loudness range: {d.loudness_range_lu:.1f} LU, Max momentary: {d.max_momentary_lufs:.1f} LUFS, "
            f"Max short-term: {d.max_short_term_lufs:.1f} LUFS")


def _rg_of_r128(r, file):
    """An R128Result in the shape everything downstream of the analysis reads (gain_db, peak, gain_steps(), file_type):
    the peak is the true peak when it was asked for, the loudness is in LUFS."""
    ft = rgmod.AudioFileType.Aac if mp4meta.is_mp4_file(file) else rgmod.AudioFileType.Mp3
    res = rgmod.ReplayGainResult(r.loudness_lufs, r.gain_db, r.peak, r.sample_rate, ft, r.blocks, r.flags)
    res.loudness_lufs = r.loudness_lufs
    if r.dynamics is not None:
        res.dynamics = r.dynamics
    return res


def _file_result(file: Path, **kw) -> dict:
    d = {"file": str(file)}
    for k in _FILE_KEYS[1:]:
        if kw.get(k) is not None:
            d[k] = kw[k]
    return d


def _summary(total: int, ok: int, failed: int, dry: bool) -> dict:
    d = {"total_files": total, "successful": ok, "failed": failed}
    if dry:
        d["dry_run"] = True
    return d


def _finite(x):
    """serde_json writes non-finite floats as null."""
    if isinstance(x, float) and not math.isfinite(x):
        return None
    if isinstance(x, dict):
        return {k: _finite(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_finite(v) for v in x]
    return x


def _print_json(out, files=None, album=None, summary=None, **extra):
    files, album = _finite(files), _finite(album)
    d = {}
    if files is not None:
        d["files"] = files
    if album is not None:
        d["album"] = album
    if summary is not None:
        d["summary"] = summary
    d.update(extra)
    print(json.dumps(d, indent=2), file=out)


def _count(result: dict, tally: List[int]):
    if result.get("status") == "success":
        tally[0] += 1
    elif result.get("status") == "error":
        tally[1] += 1


def _name(p: Path) -> str:
    return p.name or "unknown"


def _file_identity(f):
    """What makes two command-line arguments the same file: device + inode (a symlink, ./x and x, a relative and an
    absolute path all name one file); the resolved path when it cannot be stat'ed."""
    try:
        st = os.stat(f)
        return (st.st_dev, st.st_ino)
    except OSError:
        return os.path.realpath(os.fspath(f))


class Cli:
    def __init__(self, opts: Options, out, err):
        self.o, self.out, self.err = opts, out, err
        self._an: Optional[rgmod.Node] = None
        self._batch: Optional[dict] = None  # results of the one batched analysis of all files (analyze_track)

    # The GPU contexts are created on first use: byte-level commands never touch a device.  The analysis runs on a node
    # (include/mp3rgain_amd_node.h): every visible GPU of the machine, one context each -- `-a` and `-r` over many files
    # deal the files out over all of them, a single file runs on the first.  MP3RGAIN_AMD_DEVICES="0,2" restricts it.
    def analyzer(self) -> rgmod.Node:
        if self._an is None:
            devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
            if devs:
                devices = [int(d) for d in devs.split(",")]
            elif len(self.o.files) <= 1:
                devices = [0]  # one file runs on one GPU: no contexts (streams, tables, pinned buffers) on the others, and a
                               # GPU that cannot be opened elsewhere on the machine does not fail a single-file command
            else:
                devices = None  # every visible GPU
            self._an = rgmod.Node(devices)
            dec = self.o.decoder or os.environ.get("MP3RGAIN_AMD_DECODER")
            if dec:
                self._an.set_decoder_command(dec)
            if self.o.surround:
                self._an.set_channel_mode_r128("layout")
        return self._an

    def analyze_track(self, file):
        """analyze_track for one file of the command line.  With several files the whole list is analysed once, as one GPU
        batch (rg_analyze_tracks: the files load on all host cores, decode and analysis run on the device), and every file
        then finds its result -- or the error it would have raised -- here; the reference analyses file by file
        (src/main.rs:1937-2001), the results are the same."""
        files = self.o.files
        if self.o.r128:
            return self._analyze_track_r128(file)
        # (a file named twice is analysed again after its first occurrence has been patched, as in the reference: no batch)
        if len(files) > 1 and len({_file_identity(f) for f in files}) == len(files):
            if self._batch is None:
                res = self.analyzer().analyze_track_files(files, self.o.track_index)
                self._batch = {os.fspath(f): r for f, r in zip(files, res)}
            r = self._batch.get(os.fspath(file))
            if r is not None:
                if isinstance(r, rgmod.ReplayGainError):
                    raise r
                return r
        return self.analyzer().analyze_track_file(file, self.o.track_index)

    def _analyze_track_r128(self, file):
        """The --r128 analysis: every file of the command line as one batch on the first GPU (the R 128 path has no node route)."""
        files = self.o.files
        an = self.analyzer().analyzer(0)
        if len(files) > 1 and len({_file_identity(f) for f in files}) == len(files):
            if self._batch is None:
                res = an.analyze_track_files_r128(files, self.o.true_peak, self.o.track_index, self.o.loudness_range)
                self._batch = {os.fspath(f): r for f, r in zip(files, res)}
            r = self._batch.get(os.fspath(file))
        else:
            r = an.analyze_track_files_r128([file], self.o.true_peak, self.o.track_index, self.o.loudness_range)[0]
        if isinstance(r, rgmod.ReplayGainError):
            raise r
        return _rg_of_r128(r, file)

    def _analyze_album_r128(self):
        a = self.analyzer().analyzer(0).analyze_album_files_r128(self.o.files, self.o.true_peak, self.o.track_index,
                                                                     self.o.loudness_range)
        album = rgmod.AlbumGainResult([_rg_of_r128(t, f) for t, f in zip(a.tracks, self.o.files)], a.loudness_lufs, a.gain_db, a.peak)
        album.loudness_lufs = a.loudness_lufs
        if a.dynamics is not None:
            album.dynamics = a.dynamics
        return album

    def _target_line(self) -> str:
        if self.o.r128:
            return "  Target: -18 LUFS (ReplayGain 2.0, EBU R 128)"
        return f"  Target: {_rust_float(REFERENCE_DB)} dB (ReplayGain 1.0)"

    def p(self, *a):
        print(*a, file=self.out)

    def e(self, *a):
        print(*a, file=self.err)

    @property
    def text(self) -> bool:
        return self.o.output_format == "text"

    @property
    def talk(self) -> bool:
        return self.text and not self.o.quiet

    # ---- run, src/main.rs:472-540 ------------------------------------------------------------------------
    def run(self) -> int:
        o = self.o
        if not o.files:
            self.e("error: no files specified")
            return 1
        if o.recursive:
            o.files = expand_files_recursive(o.files)
            if not o.files:
                self.e("error: no audio files found (MP3/M4A)")
                return 1
        if o.assume_mpeg2 and self.talk:
            self.e("note: -f (assume MPEG2) is accepted for compatibility but has no effect")
        if o.verify:
            return self.cmd_verify()
        if o.rip:
            return self.cmd_rip()
        if o.stats:
            return self.cmd_stats()
        if o.spectrum:
            return self.cmd_spectrum()
        if o.dr:
            return self.cmd_dr()
        if o.ancestry:
            return self.cmd_ancestry()
        if o.duplicates:
            return self.cmd_duplicates()
        if o.tempo:
            return self.cmd_tempo()
        if o.key:
            return self.cmd_key()
        if o.stereo:
            return self.cmd_stereo()
        if o.compare:
            return self.cmd_compare()
        if o.clicks:
            return self.cmd_clicks()
        if o.encode:
            return self.cmd_encode()
        if o.max_amplitude_only:
            return self.cmd_max_amplitude()
        if o.stored_tag_mode == "delete":
            return self.cmd_delete_tags()
        if o.stored_tag_mode == "check":
            return self.cmd_check_tags()
        if o.undo:
            return self.cmd_undo()
        if o.album_gain and not o.skip_album:
            return self.cmd_album_gain()
        if o.track_gain or o.skip_album:
            return self.cmd_track_gain()
        if o.channel_gain is not None:
            return self.cmd_apply_channel(*o.channel_gain)
        if o.gain_steps is not None:
            return self.cmd_apply(o.gain_steps)
        return self.cmd_info()

    # ---- --verify (not in the reference): what `flac -t` gives, on the GPU -----------------------------------------
    @staticmethod
    def _is_mpeg(file) -> bool:
        """What --verify sends to rg_mp3_verify: a bare MPEG Layer III stream, judged from the file's head (an ID3v2 tag and
        64 KiB behind it).  Anything else, unreadable files included, goes to rg_flac_verify as before."""
        from . import mp3verify

        try:
            with open(file, "rb") as f:
                head = f.read(10)
                want = 1 << 16
                if len(head) == 10 and head[:3] == b"ID3" and not any(b & 0x80 for b in head[6:10]):
                    want += (head[6] << 21) | (head[7] << 14) | (head[8] << 7) | head[9]
                head += f.read(want)
        except OSError:
            return False
        return mp3verify.is_mpeg(head)

    def cmd_verify(self) -> int:
        """Every file decoded by the route the analysis uses, on the first GPU.  FLAC (rg_flac_verify): the MD5 of its PCM
        compared with the signature in its STREAMINFO.  MPEG Layer III (rg_mp3_verify): dropped frames, frame CRCs, and the
        LAME extension's music length, music CRC and tag CRC.  Exit status 0 only when no file fails; a file without a
        signature or checksum does not fail.  TSV, one row per file and no header: a FLAC row is `file, verdict, frames,
        total samples, dropped frames, stored MD5, decoded MD5`; an MP3 row is `file, verdict, "mp3", audio frames, Xing frames,
        dropped frames, failed frame CRCs, stored music CRC, computed music CRC`, told apart by the word in its third field."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        is_mp3 = [self._is_mpeg(f) for f in o.files]
        res = [None] * len(o.files)
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            flac_at = [i for i, m in enumerate(is_mp3) if not m]
            mp3_at = [i for i, m in enumerate(is_mp3) if m]
            if flac_at or not mp3_at:
                for i, r in zip(flac_at, an.verify_flac([o.files[i] for i in flac_at])):
                    res[i] = r
            if mp3_at:
                for i, r in zip(mp3_at, an.verify_mp3([o.files[i] for i in mp3_at])):
                    res[i] = r
        if self.talk:
            self.p(f"mp3rgain Verifying {len(o.files)} {'' if any(is_mp3) else 'FLAC '}file(s)")
            self.p()
        results, failed = [], 0
        for file, r, mp3 in zip(o.files, res, is_mp3):
            if mp3:
                verdict, bad = r.verdict, r.failed
                failed += bad
                if o.output_format == "json":
                    d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                    if r.error is not None:
                        d["error"] = str(r.error)
                    else:
                        d.update(verdict=verdict, verified=r.verified, **r.as_dict())
                    results.append(d)
                elif o.output_format == "tsv":
                    # the third field names the kind: a FLAC row (below, unchanged) has a frame count there, never a word
                    self.p(f"{_name(file)}\t{verdict}\tmp3\t{r.audio_frames}\t{r.xing_frames}\t{r.dropped_frames}\t{r.frame_crc_failed}\t"
                           f"{r.music_crc_stored:04x}\t{r.music_crc_computed:04x}")
                elif bad or not o.quiet:
                    (self.e if r.error is not None else self.p)(f"{_name(file)} - {verdict}")
                continue
            if r.error is not None:
                verdict = str(r.error)
            elif r.dropped_frames:
                verdict = f"{r.dropped_frames} frames dropped"
            elif r.has_signature and not r.md5_match:
                verdict = "MD5 mismatch"
            elif not r.length_match:
                verdict = "length mismatch"
            elif not r.has_signature:
                verdict = "no signature"
            else:
                verdict = "verified"
            bad = verdict not in ("verified", "no signature")
            failed += bad
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdict=verdict, verified=r.verified, has_signature=r.has_signature, md5_match=r.md5_match,
                             length_match=r.length_match, complete=r.complete, frames=r.frames, total_samples=r.total_samples,
                             dropped_frames=r.dropped_frames, md5_stream=r.md5_stream.hex(), md5_decoded=r.md5_decoded.hex())
                results.append(d)
            elif o.output_format == "tsv":
                self.p(f"{_name(file)}\t{verdict}\t{r.frames}\t{r.total_samples}\t{r.dropped_frames}\t{r.md5_stream.hex()}\t{r.md5_decoded.hex()}")
            elif bad or not o.quiet:
                (self.e if r.error is not None else self.p)(f"{_name(file)} - {verdict}")
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
        return 1 if failed else 0

    # ---- --rip (not in the reference): the checksums a CD ripper's log holds, on the GPU -------------------------------
    def cmd_rip(self) -> int:
        """The files are the tracks of one disc, in order (rg_rip_checksums, the first flagged first and the last last): per
        file the CRC-32 of its PCM, the CRC-32 without null samples and the AccurateRip v1 / v2 signatures, from one decode on
        the first GPU.  With --rip-log the log's track sections are compared with the files in order.  Exit status 1 when a
        file fails, a log value mismatches, or the number of sections differs from the number of files.  TSV, one row per file
        and no header: `file, status, frames, null samples, CRC32, CRC32 without nulls, ARv1, ARv2` and, with a log, its
        verdict.  With --rip-offsets (rg_rip_offset_signatures) the AccurateRip signatures are also computed at every sample
        offset within +-2939, and the one offset at which every logged signature is the computed one is looked for
        (riplog.find_offset).  At offset 0, or without a common offset, the verdicts are those above; at another offset the
        AccurateRip checks are made there, the CRCs -- which are over other samples -- are not comparable, and the exit status
        is 0.  Text, TSV (a last row `offset`) and JSON (`offset`) say which offset it was."""
        from . import riplog

        o = self.o
        sections = None
        if o.rip_log is not None:
            try:
                sections = riplog.parse(Path(o.rip_log).read_bytes())
            except OSError as ex:
                self.e(f"error: cannot read {o.rip_log}: {ex.strerror or ex}")
                return 1
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        search = table = None
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            if o.rip_offsets:
                try:
                    table = an.rip_offset_signatures(o.files, disc=True)
                    res = table.tracks
                    search = riplog.find_offset(sections, table)
                except rgmod.ReplayGainError as ex:
                    if ex.code != -10:  # RG_ERR_REFUSED: a file takes no part, or the disc is too large: no search, the files' own outcomes
                        raise
                    self.e(f"warning: no offset search: {ex}")
            if table is None:
                res = an.rip_checksums(o.files, disc=True)
        shift = search.offset if search is not None and search.offset else 0
        if self.talk:
            self.p(f"mp3rgain Rip checksums of {len(o.files)} file(s), taken as one disc")
            self.p()
        results, failed = [], 0
        count_differs = sections is not None and len(sections) != len(o.files)
        for i, (file, r) in enumerate(zip(o.files, res)):
            verdict = None
            if sections is not None and r.error is None:
                if i < len(sections):
                    verdict = riplog.compare_at(sections[i], shift, *table.at(i, shift)) if shift else riplog.compare(sections[i], r)
            bad = r.error is not None or (verdict is not None and not verdict.ok) or (sections is not None and r.error is None and verdict is None)
            failed += bad
            vtext = None if sections is None or r.error is not None else (verdict.text if verdict is not None else "no log section")
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(frames=r.frames, sample_rate=r.sample_rate, null_samples=r.null_samples, dropped_frames=r.dropped_frames,
                             first_track=r.first_track, last_track=r.last_track, cd_rate=r.cd_rate, cd_frames=r.cd_frames,
                             complete=r.complete, crc32=f"{r.crc32:08X}", crc32_nonnull=f"{r.crc32_nonnull:08X}",
                             arv1=f"{r.arv1:08X}", arv2=f"{r.arv2:08X}")
                    if vtext is not None:
                        d["log"] = vtext
                        if verdict is not None:
                            d["log_checks"] = [{"name": n, "logged": f"{v:08X}", "ok": ok} for n, v, _, ok in verdict.checks]
                            if shift:
                                d["offset"] = shift
                                for c, (_, _, _, ok) in zip(d["log_checks"], verdict.checks):
                                    c["text"] = verdict.check_text(ok)
                results.append(d)
            elif o.output_format == "tsv":
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                else:
                    row = f"{_name(file)}\tok\t{r.frames}\t{r.null_samples}\t{r.crc32:08X}\t{r.crc32_nonnull:08X}\t{r.arv1:08X}\t{r.arv2:08X}"
                    self.p(row + (f"\t{vtext}" if vtext is not None else ""))
            elif r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            else:
                notes = [] if r.complete else [f"{r.dropped_frames} frames dropped"]
                if not r.cd_rate:
                    notes.append(f"{r.sample_rate} Hz")
                if not r.cd_frames:
                    notes.append("not a whole number of sectors")
                self.p(f"{_name(file)} - CRC32 {r.crc32:08X}  w/o null {r.crc32_nonnull:08X}  ARv1 {r.arv1:08X}  ARv2 {r.arv2:08X}"
                       + (f"  [{', '.join(notes)}]" if notes else "") + (f"  log: {vtext}" if vtext is not None else ""))
        if count_differs:
            self.e(f"error: {o.rip_log} has {len(sections)} track section(s) for {len(o.files)} file(s)")
        if o.output_format == "json":
            extra = {"offset": search.offset, "offset_search": search.text} if search is not None else {}
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False), **extra)
        elif search is not None and o.output_format == "tsv":
            self.p("offset\t" + ("none" if search.offset is None else str(search.offset)))
        elif search is not None:
            self.p(f"log: {search.text}")
        return 1 if failed or count_differs else 0

    # ---- --stats (not in the reference): what is wrong with the audio itself, on the GPU ------------------------------
    @staticmethod
    def _clock(sample: int, rate: int) -> str:
        """A sample position as m:ss.mmm."""
        ms = sample * 1000 // rate if rate else 0
        return f"{ms // 60000}:{ms // 1000 % 60:02d}.{ms % 1000:03d}"

    def cmd_stats(self) -> int:
        """Every file decoded by the route the analysis uses and scanned on the first GPU (rg_pcm_stats): per channel the peak,
        the DC offset, clipped samples and clip runs, the bits in use, dropouts, and per file the digital silence at its edges.
        The findings are a report: exit status 1 only when a file fails or has dropped frames.  TSV, no header: a row per file
        `file, verdicts, frames, sample rate, channels, bits, effective bits, lead silence, trail silence, dropped frames` and a
        row per channel `file, "ch", index, peak, DC offset, clipped, clip runs, longest clip run, first clip run, zeros, dropouts,
        longest dropout`, told apart by the word in the second field (a failing file: `file, error text`)."""
        o = self.o
        clip_run = 3 if o.clip_run is None else o.clip_run
        zero_run = 64 if o.zero_run is None else o.zero_run
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            res = an.pcm_stats(o.files, clip_run, zero_run)
        if self.talk:
            self.p(f"mp3rgain PCM stats of {len(o.files)} file(s): clip runs from {clip_run} samples, dropouts from {zero_run}")
            self.p()
        results, failed = [], 0
        for file, r in zip(o.files, res):
            bad = r.error is not None or not r.complete
            failed += bad
            words = r.verdicts
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=words, frames=r.frames, sample_rate=r.sample_rate, bits=r.bits, effective_bits=r.effective_bits,
                             float=r.bits == 0, lead_silence_frames=r.lead_silence_frames, trail_silence_frames=r.trail_silence_frames,
                             dropped_frames=r.dropped_frames, clipped=r.clipped, dropout=r.dropout, padded=r.padded, nonfinite=r.nonfinite,
                             silent=r.silent, complete=r.complete,
                             channels=[{"peak": c.peak, "min": c.min, "max": c.max, "dc_offset": c.dc_offset, "sum": c.sum, "or_mask": f"{c.or_mask:08X}",
                                        "effective_bits": c.effective_bits, "clipped": c.clipped, "clip_runs": c.clip_runs,
                                        "longest_clip_run": c.longest_clip_run,
                                        "first_clip_run": c.first_clip_run if c.clip_runs else None, "zeros": c.zeros, "lead_zeros": c.lead_zeros,
                                        "trail_zeros": c.trail_zeros, "zero_runs": c.zero_runs, "longest_zero_run": c.longest_zero_run,
                                        "nonfinite": c.nonfinite} for c in r.channels])
                results.append(d)
            elif o.output_format == "tsv":
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{','.join(words)}\t{r.frames}\t{r.sample_rate}\t{len(r.channels)}\t{r.bits}\t{r.effective_bits}\t"
                       f"{r.lead_silence_frames}\t{r.trail_silence_frames}\t{r.dropped_frames}")
                for k, c in enumerate(r.channels):
                    self.p(f"{_name(file)}\tch\t{k}\t{c.peak:.6f}\t{c.dc_offset:+.6f}\t{c.clipped}\t{c.clip_runs}\t{c.longest_clip_run}\t"
                           f"{c.first_clip_run if c.clip_runs else ''}\t{c.zeros}\t{c.zero_runs}\t{c.longest_zero_run}")
            elif r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            elif bad or not o.quiet:
                width = "float" if r.bits == 0 else f"{r.effective_bits} of {r.bits} bits"
                self.p(f"{_name(file)} - {', '.join(words)}  [{width}, silence {r.lead_silence_frames} + {r.trail_silence_frames} frames"
                       + (f", {r.dropped_frames} frames dropped" if r.dropped_frames else "") + "]")
                for k, c in enumerate(r.channels):
                    first = f" first at {self._clock(c.first_clip_run, r.sample_rate)}" if c.clip_runs else ""
                    self.p(f"    ch {k}: peak {c.peak:.6f}  DC {c.dc_offset:+.6f}  clipped {c.clipped} in {c.clip_runs} run(s){first}"
                           f"  dropouts {c.zero_runs}" + (f" (longest {c.longest_zero_run})" if c.zero_runs else "")
                           + (f"  non-finite {c.nonfinite}" if c.nonfinite else ""))
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
        return 1 if failed else 0

    # ---- --spectrum (not in the reference): where the spectrum ends, on the GPU -----------------------------------------
    def cmd_spectrum(self) -> int:
        """Every file decoded by the route the analysis uses and transformed on the first GPU (rg_spectrum): per channel the
        frequency above which there is nothing, the depth of the edge there, the frames analysed and skipped.  The findings are
        a report: exit status 1 only when a file fails or has dropped frames.  TSV, no header: a row per file `file, verdicts,
        cutoff Hz (the record's: the maximum over the channels), edge dB (of the band-limited channel with the lowest cutoff, 0
        without one), frames, sample rate, channels, dropped frames` and a row per channel `file, "ch", index, cutoff Hz,
        edge dB, analysed frames, skipped frames, flags`, told apart by the word in the second field (a failing file: `file,
        error text`).  JSON adds per channel the 256 band levels in dB relative to the loudest band (null for an empty band)."""
        o = self.o
        want_bands = o.output_format == "json"
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            res = an.spectrum(o.files, o.edge_db, o.min_cutoff, bands=want_bands)
        if self.talk:
            self.p(f"mp3rgain spectrum of {len(o.files)} file(s): edges of at least {30.0 if o.edge_db is None else o.edge_db:g} dB "
                   f"above {4000.0 if o.min_cutoff is None else o.min_cutoff:g} Hz")
            self.p()
        results, failed = [], 0
        for file, r in zip(o.files, res):
            bad = r.error is not None or not r.complete
            failed += bad
            words = r.verdicts
            flag_words = lambda c: ",".join(w for w, on in (("bandlimited", c.bandlimited), ("upsampled", c.upsampled)) if on) or "ok"  # noqa: E731
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=words, summary=r.words, cutoff_hz=r.cutoff_hz, edge_db=r.edge_db, frames=r.frames, sample_rate=r.sample_rate,
                             dropped_frames=r.dropped_frames, bandlimited=r.bandlimited, upsampled=r.upsampled, short=r.short,
                             nonfinite=r.nonfinite, complete=r.complete,
                             channels=[{"cutoff_hz": c.cutoff_hz, "edge_db": c.edge_db, "analysed_frames": c.analysed_frames,
                                        "skipped_frames": c.skipped_frames, "bandlimited": c.bandlimited, "upsampled": c.upsampled,
                                        "band_hz": r.sample_rate * 8 / 4096,
                                        "levels_db": [None if x == float("-inf") else round(x, 2) for x in c.levels_db]} for c in r.channels])
                results.append(d)
            elif o.output_format == "tsv":
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{','.join(words)}\t{r.cutoff_hz:.1f}\t{r.edge_db:.1f}\t{r.frames}\t{r.sample_rate}\t{len(r.channels)}\t"
                       f"{r.dropped_frames}")
                for k, c in enumerate(r.channels):
                    self.p(f"{_name(file)}\tch\t{k}\t{c.cutoff_hz:.1f}\t{c.edge_db:.1f}\t{c.analysed_frames}\t{c.skipped_frames}\t{flag_words(c)}")
            elif r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            elif bad or not o.quiet:
                self.p(f"{_name(file)} - {', '.join(words)}  [{r.sample_rate} Hz"
                       + (f", {r.dropped_frames} frames dropped" if r.dropped_frames else "") + "]")
                self.p(f"    {r.words}")
                for k, c in enumerate(r.channels):
                    self.p(f"    ch {k}: cutoff {c.cutoff_hz:.0f} Hz  edge {c.edge_db:.1f} dB  frames {c.analysed_frames}"
                           + (f" (+{c.skipped_frames} skipped)" if c.skipped_frames else "") + f"  {flag_words(c)}")
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
        return 1 if failed else 0

    # ---- --dr (not in the reference): the dynamic range figure, on the GPU ------------------------------------------------
    def cmd_dr(self) -> int:
        """Every file decoded by the route the analysis uses and measured on the first GPU (rg_dynamic_range): the DR figure, the
        peak and the RMS level (with the meter's factor 2) per file and per channel, and the album's figure when more than one
        file was given.  The figure follows the published description of the TT DR meter and is unverified against it.  A
        report: exit status 1 only when a file fails or has dropped frames.  TSV, no header: a row per file `file, verdicts, DR,
        DR mean, peak dB, RMS dB, frames, sample rate, channels, block frames, dropped frames`, a row per channel `file, "ch",
        index, DR, peak dB, RMS dB, peak, second peak, blocks, top blocks, non-finite` and, for more than one file, a last row
        `album, DR` (a failing file: `file, error text`); silence has no level: `-inf`, and null in JSON."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            res = an.dynamic_range(o.files, None, o.dr_top)
        album = rgmod.album_dr(res) if len(o.files) > 1 else None
        if self.talk:
            self.p(f"mp3rgain dynamic range of {len(o.files)} file(s): 3-second blocks, the loudest {200 if o.dr_top is None else o.dr_top} per mille"
                   " (after the published description of the TT DR meter; unverified against it)")
            self.p()
        num = lambda x: None if x == float("-inf") else x  # noqa: E731
        results, failed = [], 0
        for file, r in zip(o.files, res):
            bad = r.error is not None or not r.complete
            failed += bad
            words = r.verdicts
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=words, dr=r.dr, dr_mean=r.dr_mean, peak_db=num(r.peak_db), rms_db=num(r.rms_db), frames=r.frames,
                             sample_rate=r.sample_rate, block_frames=r.block_frames, dropped_frames=r.dropped_frames, silent=r.silent,
                             short=r.short, nonfinite=r.nonfinite, complete=r.complete,
                             channels=[{"dr": c.dr, "peak_db": num(c.peak_db), "rms_db": num(c.rms_db), "top_ms": c.top_ms,
                                        "mean_square": c.mean_square, "peak": c.peak, "peak2": c.peak2, "blocks": c.blocks,
                                        "top_blocks": c.top_blocks, "nonfinite": c.nonfinite} for c in r.channels])
                results.append(d)
            elif o.output_format == "tsv":
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{','.join(words)}\t{r.dr}\t{r.dr_mean:.2f}\t{r.peak_db:.2f}\t{r.rms_db:.2f}\t{r.frames}\t{r.sample_rate}\t"
                       f"{len(r.channels)}\t{r.block_frames}\t{r.dropped_frames}")
                for k, c in enumerate(r.channels):
                    self.p(f"{_name(file)}\tch\t{k}\t{c.dr:.2f}\t{c.peak_db:.2f}\t{c.rms_db:.2f}\t{c.peak}\t{c.peak2}\t{c.blocks}\t{c.top_blocks}\t"
                           f"{c.nonfinite}")
            elif r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            else:
                notes = [w for w in words if w != "ok"] + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
                self.p(f"DR{r.dr:<3d} {r.peak_db:8.2f} dB peak {r.rms_db:8.2f} dB RMS   {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
                if not o.quiet:
                    for k, c in enumerate(r.channels):
                        self.p(f"    ch {k}: DR {c.dr:.2f}  peak {c.peak_db:.2f} dB  RMS {c.rms_db:.2f} dB  blocks {c.top_blocks} of {c.blocks}"
                               + (f"  non-finite {c.nonfinite}" if c.nonfinite else ""))
        if o.output_format == "json":
            extra = {"album_dr": album} if len(o.files) > 1 else {}
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False), **extra)
        elif len(o.files) > 1 and o.output_format == "tsv":
            self.p("album\t" + ("" if album is None else str(album)))
        elif len(o.files) > 1:
            self.p("album DR" + ("  none: no complete track" if album is None else f"{album}"))
        return 1 if failed else 0

    # ---- --ancestry (not in the reference): is this PCM a decoded MP3?  On the GPU ------------------------------------------
    def cmd_ancestry(self) -> int:
        """Every file decoded by the route the analysis uses and, on the first GPU (rg_ancestry), put through the MP3 encoder's
        filterbank at all 576 alignments: per file `mp3 grid at +R (z, xISO[, mid/side])` or `no grid found` and the name, per
        view the numbers.  The verdict is a convention of this project, tried on its own encoder's streams only; "no grid
        found" proves nothing (finely coded streams, short blocks, other codecs, processed audio are not found).  A report:
        exit status 1 only when a file fails or has dropped frames.  TSV, no header: a row per file `file, verdicts, grid
        offset (empty without a grid), z, iso, best view, frames, sample rate, channels, segments, granules, dropped frames`, a
        row per view `file, "view", name, offset, ratio, second, p0, z, iso, small, active, flagged, non-finite` (a failing
        file: `file, error text`); an infinite iso is `inf`, and null in JSON."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            res = an.ancestry(o.files, o.ancestry_segments, o.ancestry_granules)
        if self.talk:
            self.p(f"mp3rgain ancestry scan of {len(o.files)} file(s): an MP3 granule grid at any of 576 alignments"
                   " (a convention of this project, held to no other checker; no grid found is no proof of lossless origin)")
            self.p()
        num = lambda x: None if x in (float("inf"), float("-inf")) else x  # noqa: E731
        results, failed = [], 0
        for file, r in zip(o.files, res):
            bad = r.error is not None or not r.complete
            failed += bad
            words = r.verdicts
            if o.output_format == "json":
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=words, mp3_grid=r.mp3_grid, grid_offset=r.grid_offset if r.mp3_grid else None, z=r.z, iso=num(r.iso),
                             midside=r.midside, best_view=None if r.best_view is None else r.views[r.best_view].name, frames=r.frames,
                             sample_rate=r.sample_rate, segments=r.segments, granules=r.granules, dropped_frames=r.dropped_frames, silent=r.silent,
                             short=r.short, nonfinite=r.nonfinite, complete=r.complete,
                             views=[{"view": v.name, "offset": v.offset, "ratio": v.ratio, "second": v.second, "p0": v.p0, "z": v.z, "iso": num(v.iso),
                                     "small": v.small, "active": v.active, "active_total": v.active_total, "flagged": v.flagged,
                                     "nonfinite": v.nonfinite} for v in r.views])
                results.append(d)
            elif o.output_format == "tsv":
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{','.join(words)}\t{r.grid_offset if r.mp3_grid else ''}\t{r.z:.2f}\t{r.iso:.3f}\t"
                       f"{'' if r.best_view is None else r.views[r.best_view].name}\t{r.frames}\t{r.sample_rate}\t{sum(1 for v in r.views if v.kind < 8)}\t"
                       f"{r.segments}\t{r.granules}\t{r.dropped_frames}")
                for v in r.views:
                    self.p(f"{_name(file)}\tview\t{v.name}\t{v.offset}\t{v.ratio:.5f}\t{v.second:.5f}\t{v.p0:.5f}\t{v.z:.2f}\t{v.iso:.3f}\t{v.small}\t"
                           f"{v.active}\t{int(v.flagged)}\t{v.nonfinite}")
            elif r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            else:
                notes = [w for w in words if w not in ("ok", "mp3-grid", "mid/side")] + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
                self.p(f"{r.summary}   {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
                if not o.quiet:
                    for v in r.views:
                        self.p(f"    {v.name}: +{v.offset}  {100.0 * v.ratio:.1f} % small (next {100.0 * v.second:.1f} %, others {100.0 * v.p0:.1f} %)"
                               f"  z {v.z:.1f}  x{v.iso:.2f}" + ("  *" if v.flagged else "") + (f"  non-finite {v.nonfinite}" if v.nonfinite else ""))
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
        return 1 if failed else 0

    # ---- --duplicates (not in the reference): which of these files are the same recording?  On the GPU ---------------------
    def cmd_duplicates(self) -> int:
        """Every file decoded by the route the analysis uses and fingerprinted on the first GPU, then every pair matched at every
        lag within the radius (rg_same_recording).  Text: a paragraph per group of more than one file, every member with its
        lag in seconds and the share of differing bits against the group's first file (`via` another member when the two did not
        match directly), and a closing `N files, G groups of duplicates`.  The fingerprint and the threshold are conventions
        of this project, measured on its own synthetic material only.  A report: exit status 1 only when a file fails or has
        dropped frames.  TSV, no header: a row per file `file, group (the index of its first member), verdicts, codes,
        matches, frames, sample rate, dropped frames` (a failing file: `file, error text`) and a row per matching pair `"pair",
        file i, file j, lag of j in seconds, differing bits, bits, per mille`."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        any_rate = o.dup_any_rate  # every file at 11025 Hz first (rg_same_recording_xrate): a code is 46.4 ms for every file
        radius = None if o.dup_radius is None else dup_radius_codes(o.dup_radius, _capi.RS_RATE_OUT if any_rate else 44100.0)
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            if any_rate:
                recs, pairs, groups = an.same_recording_any_rate(o.files, radius=radius, max_ber_permille=o.dup_ber)
            else:
                recs, pairs, groups = an.same_recording(o.files, radius=radius, max_ber_permille=o.dup_ber)

        def code_rate(k):  # the rate a code of file k counts 512 samples of
            return _capi.RS_RATE_OUT if any_rate else recs[k].sample_rate

        if self.talk:
            self.p(f"mp3rgain duplicate search among {len(o.files)} file(s): sub-band fingerprints, every pair at every offset"
                   " (a convention of this project, compatible with no other fingerprint)")
            self.p()
        failed = sum(1 for r in recs if r.error is not None or not r.complete)
        by = {(p.i, p.j): p for p in pairs}

        def against(first, k):  # -> (lag of file k against `first` in seconds, share of differing bits) or None
            p = by.get((first, k))
            return None if p is None else (p.lag_of_j * 512.0 / code_rate(k), p.ber)

        if o.output_format == "json":
            files = []
            for i, (file, r) in enumerate(zip(o.files, recs)):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=r.verdicts, group=r.group, matches=r.matches, codes=r.codes, frames=r.frames, sample_rate=r.sample_rate,
                             channels=r.channels, dropped_frames=r.dropped_frames, nonfinite_frames=r.nonfinite_frames, complete=r.complete)
                files.append(d)
            _print_json(self.out, files=files,
                        pairs=[{"i": p.i, "j": p.j, "lag_codes": p.lag_of_j, "lag_seconds": p.lag_of_j * 512.0 / code_rate(p.j),
                                "errors": p.errors, "bits": p.bits, "ber": p.ber} for p in pairs],
                        groups=[[str(o.files[k]) for k in g] for g in groups],
                        summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(o.files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                else:
                    self.p(f"{_name(file)}\t{r.group}\t{','.join(r.verdicts)}\t{r.codes}\t{r.matches}\t{r.frames}\t{r.sample_rate}\t{r.dropped_frames}")
            for p in pairs:
                self.p(f"pair\t{_name(o.files[p.i])}\t{_name(o.files[p.j])}\t{p.lag_of_j * 512.0 / code_rate(p.j):.3f}\t{p.errors}\t{p.bits}\t"
                       f"{1000.0 * p.ber:.1f}")
            return 1 if failed else 0
        for file, r in zip(o.files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
            elif r.verdicts != ["ok"] and not o.quiet:
                notes = r.verdicts + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
                self.p(f"{_name(file)}  [{', '.join(notes)}]")
        for n, g in enumerate(groups, 1):
            self.p(f"group {n}: {len(g)} files")
            self.p(f"    {_name(o.files[g[0]])}" + (f"   {recs[g[0]].sample_rate} Hz" if any_rate else ""))
            for k in g[1:]:
                a = against(g[0], k)
                self.p(f"    {_name(o.files[k])}   " + (f"{recs[k].sample_rate} Hz   " if any_rate else "") + ("via another member" if a is None else f"{a[0]:+.3f} s   {100.0 * a[1]:.1f} % of bits differ"))
            self.p()
        self.p(f"{len(o.files)} files, {len(groups)} groups of duplicates")
        return 1 if failed else 0

    # ---- --tempo (not in the reference): how fast is each file?  On the GPU -----------------------------------------------------
    def cmd_tempo(self) -> int:
        """Every file decoded by the route the analysis uses; its onset curve, the windowed autocorrelation and the beat grid on
        the first GPU (rg_tempo).  Text: a line per file, `128.00 BPM  (confidence 0.89, steady 1.00, first beat 0.157 s)  name`
        or `no tempo found  name`, with the verdicts in brackets when there are any.  The estimator is a convention of this
        project, tried on synthetic material only; the reading lies in [--tempo-min, twice that).  A report: exit status 1 only
        when a file fails or has dropped frames.  TSV, no header: a row per file `file, bpm, confidence, steady, first beat in
        seconds, verdicts, period16, onsets, windows, frames, sample rate, dropped frames` (a failing file: `file, error text`)."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.tempo(o.files, min_bpm=o.tempo_min)
        failed = sum(1 for r in recs if r.error is not None or not r.complete)
        if o.output_format == "json":
            files = []
            for file, r in zip(o.files, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(bpm=r.bpm, confidence=r.confidence, steady=r.steady, first_beat_seconds=r.first_beat_seconds, first_beat=r.first_beat if r.found else None,
                             period16=r.period16, harmonics=r.harmonics, verdicts=r.verdicts, onsets=r.onsets, windows=r.windows, frames=r.frames,
                             sample_rate=r.sample_rate, channels=r.channels, dropped_frames=r.dropped_frames, nonfinite_frames=r.nonfinite_frames,
                             complete=r.complete)
                files.append(d)
            _print_json(self.out, files=files, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(o.files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                reading = f"{r.bpm:.3f}\t{r.confidence:.3f}\t{r.steady:.3f}\t{r.first_beat_seconds:.3f}" if r.found else "\t\t\t"
                self.p(f"{_name(file)}\t{reading}\t{','.join(r.verdicts)}\t{r.period16}\t{r.onsets}\t{r.windows}\t{r.frames}\t{r.sample_rate}\t{r.dropped_frames}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain tempo of {len(o.files)} file(s): onset curve and windowed autocorrelation"
                   " (a convention of this project, tried on synthetic material only)")
            self.p()
        for file, r in zip(o.files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            notes = [v for v in r.verdicts if v not in ("ok", "none")] + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
            self.p(f"{tempo_line(r)}  {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
        return 1 if failed else 0

    # ---- --key (not in the reference): in which key is each file?  On the GPU --------------------------------------------------
    def cmd_key(self) -> int:
        """Every file decoded by the route the analysis uses; its signal decimated to 5 .. 10 kHz, a chroma row per 512 decimated
        samples and the match against the Krumhansl-Kessler profiles on the first GPU (rg_key).  Text: a line per file,
        `A minor  (8A, correlation 0.93, margin 0.27, steady 1.00)  name` or `no key found  name`, with the verdicts in brackets
        when there are any.  The estimator is a convention of this project, tried on synthetic material only.  A report: exit
        status 1 only when a file fails or has dropped frames.  TSV, no header: a row per file `file, key, camelot, open key,
        correlation, margin, steady, verdicts, key number, rows, segments, frames, sample rate, dropped frames` (a failing file:
        `file, error text`)."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.key(o.files, segment=o.key_segment)
        failed = sum(1 for r in recs if r.error is not None or not r.complete)
        if o.output_format == "json":
            files = []
            for file, r in zip(o.files, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(key=r.name, camelot=r.camelot, open_key=r.open_key, key_number=r.key if r.found else None, tonic=r.tonic if r.found else None,
                             mode=("minor" if r.mode else "major") if r.found else None, correlation=r.correlation, margin=r.margin, steady=r.steady,
                             verdicts=r.verdicts, rows=r.rows, silent_rows=r.silent_rows, segments=r.segments, decim=r.decim, frames=r.frames,
                             sample_rate=r.sample_rate, channels=r.channels, dropped_frames=r.dropped_frames, nonfinite_frames=r.nonfinite_frames,
                             complete=r.complete)
                files.append(d)
            _print_json(self.out, files=files, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(o.files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                reading = f"{r.name}\t{r.camelot}\t{r.open_key}\t{r.correlation:.3f}\t{r.margin:.3f}\t{r.steady:.3f}" if r.found else "\t\t\t\t\t"
                self.p(f"{_name(file)}\t{reading}\t{','.join(r.verdicts)}\t{r.key if r.found else ''}\t{r.rows}\t{r.segments}\t{r.frames}\t{r.sample_rate}\t{r.dropped_frames}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain key of {len(o.files)} file(s): decimated chromagram and key-profile match"
                   " (a convention of this project, tried on synthetic material only)")
            self.p()
        for file, r in zip(o.files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            notes = [v for v in r.verdicts if v not in ("ok", "none")] + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
            self.p(f"{key_line(r)}  {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
        return 1 if failed else 0

    # ---- --stereo (not in the reference): how do the two channels of each file relate?  On the GPU ----------------------------
    def cmd_stereo(self) -> int:
        """Every file decoded by the route the analysis uses; the moments of channels 0 and 1, the raw comparisons and the
        cross-correlation at every lag within the radius on the first GPU (rg_stereo).  Text: a line per file, `stereo
        (correlation 0.62, side -7.1 dB, balance +0.3 dB)  name`, `dual mono  name`, `right channel late by 3 samples (correlation
        0.998 there, 0.41 in place)  name`, `channels out of phase  (...)  name`, `mono file  name`, with the other verdicts in
        brackets.  The definitions are a convention of this project, tried on synthetic material only.  A report: exit status 1
        only when a file fails or has dropped frames.  TSV, no header: a row per file `file, verdicts, correlation, side dB,
        balance dB, lag, lag correlation, anti lag, anti correlation, frames, sample rate, channels, radius, dropped frames` (a
        failing file: `file, error text`)."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.stereo(o.files, radius=o.stereo_radius)
        failed = sum(1 for r in recs if r.error is not None or not r.complete)
        num = lambda x: x if math.isfinite(x) else None  # noqa: E731  (JSON has no infinity)
        if o.output_format == "json":
            files = []
            for file, r in zip(o.files, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=r.verdicts, reading=stereo_line(r), correlation=r.correlation, lag_correlation=r.lag_correlation,
                             anti_correlation=r.anti_correlation, balance_db=num(r.balance_db), side_db=num(r.side_db),
                             balance=("left" if r.balance_db > 0 else "right") if math.isinf(r.balance_db) else None,
                             side=("all" if r.side_db > 0 else "none") if math.isinf(r.side_db) else None, lag=r.lag, anti_lag=r.anti_lag,
                             lag_sum=r.lag_sum, anti_sum=r.anti_sum, ell=r.ell, err=r.err, elr=r.elr, equal_frames=r.equal_frames,
                             opposite_frames=r.opposite_frames, zero_frames=r.zero_frames, nonfinite=r.nonfinite, blocks=r.blocks,
                             active_blocks=r.active_blocks, neg_blocks=r.neg_blocks, mono_blocks=r.mono_blocks, block_frames=r.block_frames,
                             radius=r.radius, frames=r.frames, sample_rate=r.sample_rate, channels=r.channels, format=r.format, flags=r.flags,
                             dropped_frames=r.dropped_frames, complete=r.complete)
                files.append(d)
            _print_json(self.out, files=files, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(o.files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{','.join(r.verdicts)}\t{r.correlation:.4f}\t{r.side_db:.2f}\t{r.balance_db:.2f}\t{r.lag}\t{r.lag_correlation:.4f}\t"
                       f"{r.anti_lag}\t{r.anti_correlation:.4f}\t{r.frames}\t{r.sample_rate}\t{r.channels}\t{r.radius}\t{r.dropped_frames}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain stereo image of {len(o.files)} file(s): correlation, balance and channel delay within "
                   f"{_capi.ST_DEFAULT_RADIUS if o.stereo_radius is None else o.stereo_radius} samples"
                   " (a convention of this project, tried on synthetic material only)")
            self.p()
        named = ("stereo", "mono file", "silent", "dual mono", "inverted copy", "delayed", "out of phase", "one-sided", "near mono")
        for file, r in zip(o.files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            line = stereo_line(r)
            shown = next((w for w in named[1:] if w in r.verdicts), "stereo")
            notes = [w for w in r.verdicts if w not in ("stereo", "incomplete", shown)] + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])
            self.p(f"{line}  {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
        return 1 if failed else 0

    # ---- --compare (not in the reference): a null test of every file against the first.  On the GPU ------------------------------
    def cmd_compare(self) -> int:
        """Every file decoded by the route the analysis uses; every file but the first lined up with the first to the sample
        (the coarse lag from the fingerprint match, or --compare-hint for all of them), one gain fitted and what is left sized, on
        the first GPU (rg_compare).  Text: a line per file but the first, `identical  name`, `identical samples, starts 588 samples
        later, 1176 shorter at the end  name`, `same master  (gain -3.01 dB, residual 0.31 LSB^2)  name`, `same recording, differs
        (null -23.4 dB after +0.2 dB, worst 1:02-1:03 at -9.1 dB, first difference at 0:00.013)  name`, `same recording, drifts
        (...)  name`, `inverted copy, ...  name`, `not the same recording  (best correlation 0.03)  name`, `different sample rate:
        not compared  name`, with the other verdicts in brackets.  The definitions are a convention of this project, held to no
        other tool.  A report: exit status 1 only when a file fails or has dropped frames.  JSON carries every field of the
        record.  TSV, no header: a row per file `file, verdicts, lag, polarity, lock, gain dB, null dB, residual LSB^2, overlap,
        a head, a tail, b head, b tail, differing blocks, first difference, max difference, sample rate, channels, dropped a,
        dropped b` (a failing file: `file, error text`)."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.compare(o.files, hints=o.compare_hint, radius=o.compare_radius)
        return self.print_compare(o.files[1:], recs)

    def print_compare(self, files, recs) -> int:
        """The report of cmd_compare: `recs[k]` is files[k] against the reference copy."""
        o = self.o
        failed = sum(1 for r in recs if r.error is not None or not r.complete)
        num = lambda x: x if math.isfinite(x) else None  # noqa: E731  (JSON has no infinity)
        if o.output_format == "json":
            out = []
            for file, r in zip(files, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    d.update(verdicts=r.verdicts, reading=r.reading, complete=r.complete)
                    for f in rgmod._COMPARE_FIELDS:
                        v = getattr(r, f)
                        d[f] = num(v) if isinstance(v, float) else v
                    d["first_diff"] = None if r.first_diff == _capi.CMP_NONE else r.first_diff
                out.append(d)
            _print_json(self.out, reference=str(o.files[0]), files=out, summary=_summary(len(files), len(files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                first = "" if r.first_diff == _capi.CMP_NONE else str(r.first_diff)
                self.p(f"{_name(file)}\t{','.join(r.verdicts)}\t{r.lag}\t{r.polarity}\t{r.lock:.4f}\t{r.gain_db:.3f}\t{r.null_db:.2f}\t{r.residual_lsb2:.4f}\t"
                       f"{r.overlap}\t{r.a_head}\t{r.a_tail}\t{r.b_head}\t{r.b_tail}\t{r.differing_blocks}\t{first}\t{r.max_diff}\t{r.sample_rate}\t"
                       f"{r.channels}\t{r.dropped_a}\t{r.dropped_b}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain null test of {len(files)} file(s) against {_name(o.files[0])}: lag, gain and what is left"
                   " (a convention of this project, held to no other tool)")
            self.p()
        shown = ("different sample rate", "no overlap", "identical", "same master", "differs", "unrelated", "inverted", "drifts", "shifted", "lengths differ",
                 "incomplete")
        for file, r in zip(files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            notes = [w for w in r.verdicts if w not in shown]
            dropped = r.dropped_a + r.dropped_b
            notes += [f"{dropped} frames dropped"] if dropped else []
            self.p(f"{r.reading}  {_name(file)}" + (f"  [{', '.join(notes)}]" if notes else ""))
        return 1 if failed else 0

    # ---- --encode (not in the reference): WAV and FLAC files to FLAC on the GPU ---------------------------------------------------
    def cmd_encode(self) -> int:
        """Every file decoded by the route the analysis uses and encoded where its PCM lies on the first GPU
        (rg_flac_encode_files) into `<--encode-dir>/<stem>.flac`; unless --no-encode-verify every stream is decoded again on the
        GPU and its MD5 held to the source's before the file is written.  Text: a line per file `name -> out  1234567 bytes,
        61.3 % of the PCM, verified`, and a closing total.  Exit status 1 for any failing file.  TSV, no header: a row per file
        `file, output, stream bytes, PCM bytes, PCM frames, FLAC frames, sample rate, channels, bits, dropped frames, verified,
        MD5` (a failing file: `file, error text`)."""
        o = self.o
        outs = [o.encode_dir / (Path(f).stem + ".flac") for f in o.files]
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.encode_flac(o.files, outs, block_size=o.encode_block, max_lpc_order=o.encode_lpc, verify=o.encode_verify)
        failed = sum(1 for r in recs if r.error is not None)
        good = [r for r in recs if r.error is None]
        total_stream, total_pcm = sum(r.stream_bytes for r in good), sum(r.pcm_bytes for r in good)
        if o.output_format == "json":
            files = []
            for file, dst, r in zip(o.files, outs, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                    d["verify_failed"] = r.verify_failed
                else:
                    d.update(output=str(dst), stream_bytes=r.stream_bytes, pcm_bytes=r.pcm_bytes, ratio=r.ratio, pcm_frames=r.pcm_frames,
                             flac_frames=r.flac_frames, sample_rate=r.sample_rate, channels=r.channels, bits_per_sample=r.bits_per_sample,
                             block_size=r.block_size, min_frame_bytes=r.min_frame_bytes, max_frame_bytes=r.max_frame_bytes,
                             metadata_bytes=r.metadata_bytes, dropped_frames=r.dropped_frames, complete=r.complete, verified=r.verified,
                             md5=r.md5_pcm.hex())
                files.append(d)
            _print_json(self.out, files=files, stream_bytes=total_stream, pcm_bytes=total_pcm,
                        summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, dst, r in zip(o.files, outs, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                self.p(f"{_name(file)}\t{dst}\t{r.stream_bytes}\t{r.pcm_bytes}\t{r.pcm_frames}\t{r.flac_frames}\t{r.sample_rate}\t{r.channels}\t"
                       f"{r.bits_per_sample}\t{r.dropped_frames}\t{int(r.verified)}\t{r.md5_pcm.hex()}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain encoding {len(o.files)} file(s) to FLAC in {o.encode_dir}" + ("" if o.encode_verify else " (not verified)"))
            self.p()
        for file, dst, r in zip(o.files, outs, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            notes = (["verified"] if r.verified else []) + ([f"{r.dropped_frames} frames of the source dropped"] if r.dropped_frames else [])
            self.p(f"{_name(file)} -> {dst}  {r.stream_bytes} bytes, {100.0 * r.ratio:.1f} % of the PCM" + "".join(", " + w for w in notes))
        if self.talk:
            self.p()
            self.p(f"{len(good)} of {len(o.files)} file(s) written: {total_stream} bytes, "
                   f"{100.0 * total_stream / total_pcm if total_pcm else 0.0:.1f} % of {total_pcm} bytes of PCM")
        return 1 if failed else 0

    # ---- --clicks (not in the reference): are there clicks or glitches in each file?  On the GPU --------------------------------
    def cmd_clicks(self) -> int:
        """Every file decoded by the route the analysis uses; every channel predicted block by block by the FLAC encoder's linear
        model, the samples whose residual stands far above the median residual around them gathered into events on the first GPU
        (rg_clicks).  Text: a line per file, `no clicks  name` or `3 clicks (first at 1:02.345 left, strongest x41.2 at 2:10.007
        right), 1 burst  name`, other findings in brackets, and under it the listed events, one per line.  The definitions are a
        convention of this project, tried on synthetic material only.  A report: exit status 1 only when a file fails or has
        dropped frames.  TSV, no header: a row per file `file, clicks, bursts, flagged samples, first click (sample), its channel,
        strongest (x), its sample, its channel, events, listed, frames, sample rate, channels, ratio, dropped frames`, then a row
        per listed event `file, kind, start, width, channel, peak sample, strength (x)` (a failing file: `file, error text`)."""
        o = self.o
        devs = os.environ.get("MP3RGAIN_AMD_DEVICES")
        ratio = None if o.click_ratio is None else int(round(o.click_ratio * 1000.0))
        with rgmod.Analyzer(int(devs.split(",")[0]) if devs else 0) as an:
            recs = an.clicks(o.files, block_samples=o.click_block, order=o.click_order, ratio_permille=ratio, max_events=o.click_list)
        failed = sum(1 for r in recs if r.error is not None or not r.complete)

        def notes(r):
            words = [w for w, bit in (("silent", _capi.CK_SILENT), ("nonfinite", _capi.CK_NONFINITE)) if r.flags & bit]
            if r.truncated and r.max_events:
                words.append(f"the first {r.listed} of {r.events_total} events listed")
            return words + ([f"{r.dropped_frames} frames dropped"] if r.dropped_frames else [])

        if o.output_format == "json":
            files = []
            for file, r in zip(o.files, recs):
                d = {"file": str(file), "status": "error" if r.error is not None else "success"}
                if r.error is not None:
                    d["error"] = str(r.error)
                else:
                    first, strongest = r.first_click, r.strongest_click
                    d.update(reading=clicks_line(r), clicks=r.clicks, bursts=r.bursts,
                             first_click=None if first is None else {"sample": first[0], "channel": first[1], "time": _click_time(first[0], r.sample_rate)},
                             strongest_click=None if strongest is None else {"strength": strongest[0] / 1000.0, "sample": strongest[1], "channel": strongest[2],
                                                                             "time": _click_time(strongest[1], r.sample_rate)},
                             channel_records=[vars(c) for c in r.ch], events=[dict(vars(e), time=_click_time(e.start, r.sample_rate)) for e in r.events],
                             events_total=r.events_total, listed=r.listed, truncated=r.truncated, nonfinite=r.nonfinite, block_samples=r.block_samples,
                             order=r.order, ratio_permille=r.ratio_permille, floor=r.floor, gap=r.gap, max_width=r.max_width, max_events=r.max_events,
                             frames=r.frames, sample_rate=r.sample_rate, channels=r.channels, format=r.format, flags=r.flags,
                             dropped_frames=r.dropped_frames, complete=r.complete)
                files.append(d)
            _print_json(self.out, files=files, summary=_summary(len(o.files), len(o.files) - failed, failed, False))
            return 1 if failed else 0
        if o.output_format == "tsv":
            for file, r in zip(o.files, recs):
                if r.error is not None:
                    self.p(f"{_name(file)}\t{r.error}")
                    continue
                first, strongest = r.first_click or ("", ""), r.strongest_click or (0, "", "")
                self.p(f"{_name(file)}\t{r.clicks}\t{r.bursts}\t{sum(c.flagged for c in r.ch)}\t{first[0]}\t{first[1]}\t{strongest[0] / 1000.0:.3f}\t{strongest[1]}\t"
                       f"{strongest[2]}\t{r.events_total}\t{r.listed}\t{r.frames}\t{r.sample_rate}\t{r.channels}\t{r.ratio_permille / 1000.0:.3f}\t{r.dropped_frames}")
                for e in r.events:
                    self.p(f"{_name(file)}\t{e.kind}\t{e.start}\t{e.width}\t{e.channel}\t{e.peak_at}\t{e.strength_permille / 1000.0:.3f}")
            return 1 if failed else 0
        if self.talk:
            self.p(f"mp3rgain click scan of {len(o.files)} file(s): residual of a linear predictor against {_capi.CK_DEFAULT_RATIO_PERMILLE / 1000.0 if ratio is None else ratio / 1000.0:g}"
                   " times its local median (a convention of this project, tried on synthetic material only)")
            self.p()
        for file, r in zip(o.files, recs):
            if r.error is not None:
                self.e(f"{_name(file)} - {r.error}")
                continue
            extra = notes(r)
            self.p(f"{clicks_line(r)}  {_name(file)}" + (f"  [{', '.join(extra)}]" if extra else ""))
            for e in r.events:
                self.p(click_event_line(e, r))
        return 1 if failed else 0

    # ---- find_max_amplitude, src/lib.rs:1174-1199 ------------------------------------------------------------
    def find_max_amplitude(self, file: Path):
        info = mp3gain.analyze(file)  # "No valid MP3 frames found" for anything that is not MP3
        peak = self.analyzer().find_peak_amplitude_file(file).peak
        return peak, info.max_gain, info.min_gain

    # ---- -x, src/main.rs:583-689 -------------------------------------------------------------------------------
    def cmd_max_amplitude(self) -> int:
        o = self.o
        if self.talk:
            self.p(f"mp3rgain Finding maximum amplitude for {len(o.files)} file(s)")
            self.p()
        results = []
        for file in o.files:
            name = _name(file)
            try:
                max_amp, max_gain, min_gain = self.find_max_amplitude(file)
            except (mp3gain.Mp3GainError, rgmod.ReplayGainError) as ex:
                if o.output_format == "json":
                    results.append(_file_result(file, status="error", error=str(ex)))
                elif not o.quiet:
                    self.e(f"{name} - {ex}")
                continue
            pcm = max_amp * 32768.0
            headroom = -20.0 * math.log10(max_amp) if max_amp > 0.0 else math.inf
            may_clip = file.suffix.lower() == ".mp3" and max_amp >= 0.9999
            if o.output_format == "text":
                if not o.quiet:
                    self.p(name)
                    self.p(f"  Max PCM sample: {pcm:.6f}")
                    if may_clip:
                        self.p("    (may be clipped - actual peak could be higher)")
                    self.p(f"  Headroom:       {_signed(headroom, 2)} dB")
                    self.p(f"  Max global_gain: {max_gain}")
                    self.p(f"  Min global_gain: {min_gain}")
                    self.p()
                else:
                    self.p(f"{name}\t{pcm:.6f}\t{_plain(headroom, 2)}")
            elif o.output_format == "tsv":
                self.p(f"{name}\t{pcm:.6f}\t{_plain(headroom, 2)}\t{max_gain}\t{min_gain}")
            else:
                results.append(_file_result(file, max_amplitude=pcm, headroom_db=headroom, max_gain=max_gain, min_gain=min_gain,
                                            warning="peak may be clipped - actual value could be higher" if may_clip else None))
        if o.output_format == "json":
            _print_json(self.out, files=results)
        return 0

    # ---- -s d, src/main.rs:691-794 -----------------------------------------------------------------------------
    def cmd_delete_tags(self) -> int:
        o = self.o
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain {'Would delete' if o.dry_run else 'Deleting'} ReplayGain tags from {len(o.files)} file(s)")
            self.p()
        results, tally = [], [0, 0]
        for file in o.files:
            name = _name(file)
            if o.dry_run:
                if self.talk:
                    self.p(f"  ~ [DRY RUN] {name} (would delete tags)")
                results.append(_file_result(file, status="dry_run", dry_run=True))
                continue
            mtime = _mtime(file) if o.preserve_timestamp else None
            try:
                mp3gain.delete_ape_tag(file)
            except mp3gain.Mp3GainError as ex:
                if self.talk:
                    self.e(f"  x {name} - {ex}")
                tally[1] += 1
                results.append(_file_result(file, status="error", error=str(ex)))
                continue
            _restore(file, mtime)
            if self.talk:
                self.p(f"  v {name} (tags deleted)")
            tally[0] += 1
            results.append(_file_result(file, status="success"))
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        elif o.dry_run and not o.quiet:
            self.p()
            self.p("No files were modified.")
        return 0

    # ---- -s c, src/main.rs:796-917 -----------------------------------------------------------------------------
    def cmd_check_tags(self) -> int:
        o = self.o
        if self.talk:
            self.p(f"mp3rgain Checking stored tag info for {len(o.files)} file(s)")
            self.p()
        results = []
        keys = ("MP3GAIN_UNDO", "MP3GAIN_MINMAX", "REPLAYGAIN_TRACK_GAIN", "REPLAYGAIN_TRACK_PEAK", "REPLAYGAIN_ALBUM_GAIN",
                "REPLAYGAIN_ALBUM_PEAK")
        for file in o.files:
            name = _name(file)
            try:
                has_tag = mp3gain.has_ape_tag(file)
                vals = [mp3gain.read_ape_tag_value(file, k) for k in keys] if has_tag else []
            except (mp3gain.Mp3GainError, OSError) as ex:
                if o.output_format != "json":
                    self.e(f"{name} - {ex}")
                else:
                    results.append(_file_result(file, status="error", error=str(ex)))
                continue
            if not has_tag:
                if self.text:
                    self.p(name)
                    self.p("  (no APE tag found)")
                    self.p()
                elif o.output_format == "tsv":
                    self.p(f"{name}\t-\t-\t-\t-\t-\t-")
                else:
                    results.append(_file_result(file, status="no_tag"))
                continue
            if self.text:
                self.p(name)
                labels = ("  MP3GAIN_UNDO:         ", "  MP3GAIN_MINMAX:       ", "  REPLAYGAIN_TRACK_GAIN: ", "  REPLAYGAIN_TRACK_PEAK: ",
                          "  REPLAYGAIN_ALBUM_GAIN: ", "  REPLAYGAIN_ALBUM_PEAK: ")
                for lab, v in zip(labels, vals):
                    if v is not None:
                        self.p(f"{lab}{v}")
                if vals[0] is None and vals[1] is None and vals[2] is None:
                    self.p("  (no mp3gain tags found)")
                self.p()
            elif o.output_format == "tsv":
                self.p("\t".join([name] + [v if v is not None else "-" for v in vals]))
            else:
                results.append(_file_result(file, status="success"))
        if o.output_format == "json":
            _print_json(self.out, files=results)
        return 0

    # ---- -g, src/main.rs:948-1033 and 1488-1616 ------------------------------------------------------------------
    def cmd_apply(self, steps: int) -> int:
        o = self.o
        if steps == 0:
            if o.output_format == "json":
                _print_json(self.out, files=[], summary=_summary(len(o.files), 0, 0, o.dry_run))
            elif not o.quiet:
                self.p("info: gain is 0, nothing to do")
            return 0
        db = steps * GAIN_STEP_DB
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain {'Would apply' if o.dry_run else 'Applying'} {steps} step(s) ({db:+.1f} dB) to {len(o.files)} file(s)")
            if o.wrap_gain:
                self.p("  ! Wrap mode enabled")
            self.p()
        results, tally = [], [0, 0]
        for file in o.files:
            r = self.process_apply(file, steps)
            _count(r, tally)
            if o.output_format == "tsv":
                try:
                    info = mp3gain.analyze(file)
                    self.p(f"{_name(file)}\t{steps}\t{db:.1f}\t{1.0:.6f}\t{info.max_gain}\t{info.min_gain}")
                except mp3gain.Mp3GainError:
                    pass
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        else:
            self._dry_run_notice()
        return 0

    def _dry_run_notice(self):  # src/main.rs:941-946
        if self.o.dry_run and self.talk:
            self.p()
            self.p("No files were modified.")

    def _with_temp_file(self, file: Path, op):  # apply_with_temp_file, src/main.rs:1458-1486
        if not self.o.use_temp_file:
            return op(file)
        tmp = (file.parent if str(file.parent) else Path(".")) / f".mp3rgain_temp_{os.getpid()}.mp3"
        shutil.copyfile(file, tmp)
        try:
            frames = op(tmp)
        except Exception:
            try:
                tmp.unlink()
            except OSError:
                pass
            raise
        os.replace(tmp, file)
        return frames

    def process_apply(self, file: Path, steps: int) -> dict:
        o = self.o
        name = _name(file)
        pre = "[DRY RUN] " if o.dry_run else ""
        mtime = _mtime(file) if o.preserve_timestamp and not o.dry_run else None
        actual, warning = steps, None
        if steps > 0 and not o.wrap_gain:
            try:
                info = mp3gain.analyze(file)
            except mp3gain.Mp3GainError:
                info = None
            if info is not None and steps > info.headroom_steps:
                if o.prevent_clipping:
                    actual = info.headroom_steps
                    if self.talk:
                        self.e(f"  ! {pre}{name} - gain reduced from {steps} to {actual} steps to prevent clipping")
                    warning = f"gain reduced from {steps} to {actual} steps to prevent clipping"
                elif not o.ignore_clipping and not o.quiet:
                    if self.text:
                        self.e(f"  ! {pre}{name} - clipping warning: requested {steps} steps but only {info.headroom_steps} headroom")
                        self.e("      Use -c to ignore clipping warnings or -k to prevent clipping")
                    warning = f"clipping warning: requested {steps} steps but only {info.headroom_steps} headroom"
        if o.dry_run:
            if self.talk:
                self.p(f"  ~ [DRY RUN] {name} (would apply {actual} steps)")
            return _file_result(file, status="dry_run", gain_applied_steps=actual, gain_applied_db=actual * GAIN_STEP_DB,
                                warning=warning, dry_run=True)
        if o.stored_tag_mode == "skip":  # -s s: no undo tag
            fn = mp3gain.apply_gain_wrap if o.wrap_gain else mp3gain.apply_gain
        else:
            fn = mp3gain.apply_gain_with_undo_wrap if o.wrap_gain else mp3gain.apply_gain_with_undo
        try:
            frames = self._with_temp_file(file, lambda f: fn(f, actual))
        except (mp3gain.Mp3GainError, OSError) as ex:
            if self.talk:
                self.e(f"  x {name} - {ex}")
            return _file_result(file, status="error", error=str(ex))
        _restore(file, mtime)
        if self.talk:
            self.p(f"  v {name} ({frames} frames)")
        return _file_result(file, status="success", frames=frames, gain_applied_steps=actual,
                            gain_applied_db=actual * GAIN_STEP_DB, warning=warning)

    # ---- -l, src/main.rs:1035-1118 and 1618-1697 -----------------------------------------------------------------
    def cmd_apply_channel(self, channel: int, steps: int) -> int:
        o = self.o
        if steps == 0:
            if o.output_format == "json":
                _print_json(self.out, files=[], summary=_summary(len(o.files), 0, 0, o.dry_run))
            elif not o.quiet:
                self.p("info: gain is 0, nothing to do")
            return 0
        db = steps * GAIN_STEP_DB
        cname = "left" if channel == 0 else "right"
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain {'Would apply' if o.dry_run else 'Applying'} {steps} step(s) ({db:+.1f} dB) to {cname} channel of {len(o.files)} file(s)")
            self.p()
        results, tally = [], [0, 0]
        for file in o.files:
            name = _name(file)
            if o.dry_run:
                if self.talk:
                    self.p(f"  ~ [DRY RUN] {name} (would apply {steps} steps to {cname} channel)")
                r = _file_result(file, status="dry_run", gain_applied_steps=steps, gain_applied_db=db, dry_run=True)
            else:
                mtime = _mtime(file) if o.preserve_timestamp else None
                try:
                    frames = mp3gain.apply_gain_channel_with_undo(file, mp3gain.Channel(channel), steps)
                    _restore(file, mtime)
                    if self.talk:
                        self.p(f"  v {name} ({frames} frames, {cname} channel)")
                    r = _file_result(file, status="success", frames=frames, gain_applied_steps=steps, gain_applied_db=db)
                except mp3gain.Mp3GainError as ex:
                    if self.talk:
                        self.e(f"  x {name} - {ex}")
                    r = _file_result(file, status="error", error=str(ex))
            _count(r, tally)
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        else:
            self._dry_run_notice()
        return 0

    # ---- default command, src/main.rs:1120-1153 and 1699-1854 ------------------------------------------------------
    def cmd_info(self) -> int:
        o = self.o
        if o.output_format == "tsv":
            self.p("File\tMP3 gain\tdB gain\tMax Amplitude\tMax global_gain\tMin global_gain")
        results = []
        for file in o.files:
            r = self.process_info(file)
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results)
        return 0

    def process_info(self, file: Path) -> dict:
        o = self.o
        name = _name(file)
        if o.output_format == "tsv":  # mp3gain-compatible TSV (what beets parses): ReplayGain analysis
            try:
                rg = self.analyze_track(file)
            except rgmod.ReplayGainError as ex:
                self.e(f"{name} - {ex}")
                return _file_result(file, status="error", error=str(ex))
            try:
                max_amp, max_gain, min_gain = self.find_max_amplitude(file)
            except (mp3gain.Mp3GainError, rgmod.ReplayGainError):
                max_amp, max_gain, min_gain = 1.0, 255, 0
            gain_db = rg.gain_db + o.gain_modifier_db  # -d shifts the suggested gain
            steps = mp3gain.db_to_steps(gain_db)
            self.p(f"{name}\t{steps}\t{gain_db:.6f}\t{rg.peak * 32768.0:.6f}\t{max_gain}\t{min_gain}")
            return _file_result(file, loudness_db=rg.loudness_db, loudness_lufs=_lufs(rg), **_dyn(rg), gain_applied_db=gain_db, gain_applied_steps=steps, peak=rg.peak,
                                max_amplitude=max_amp, max_gain=max_gain, min_gain=min_gain)
        if mp4meta.is_mp4_file(file):
            if self.text:
                if o.quiet:
                    self.p(f"{name}\tM4A/AAC\t-\t-\t-\t-\t-")
                else:
                    self.p(name)
                    self.p("  Format:      M4A/AAC")
                    self.p("  Note: Use -r or -a for ReplayGain analysis")
                    self.p()
            return _file_result(file, status="info")
        try:
            info = mp3gain.analyze(file)
        except mp3gain.Mp3GainError as ex:
            if o.output_format != "json":
                self.e(f"{name} - {ex}")
            return _file_result(file, status="error", error=str(ex))
        if self.text:
            if o.quiet:
                self.p(f"{name}\t{info.frame_count}\t{info.min_gain}\t{info.max_gain}\t{info.avg_gain:.1f}\t{info.headroom_steps}\t{info.headroom_db:.1f}")
            else:
                self.p(name)
                self.p(f"  Format:      {info.mpeg_version} Layer III, {info.channel_mode}")
                self.p(f"  Frames:      {info.frame_count}")
                self.p(f"  Gain range:  {info.min_gain} - {info.max_gain} (avg: {info.avg_gain:.1f})")
                self.p(f"  Headroom:    {info.headroom_steps} steps ({info.headroom_db:+.1f} dB)")
                self.p()
        return _file_result(file, mpeg_version=info.mpeg_version, channel_mode=info.channel_mode, frames=info.frame_count,
                            min_gain=info.min_gain, max_gain=info.max_gain, avg_gain=info.avg_gain,
                            headroom_steps=info.headroom_steps, headroom_db=info.headroom_db)

    # ---- -u, src/main.rs:1155-1211 and 1856-1935 ---------------------------------------------------------------------
    def cmd_undo(self) -> int:
        o = self.o
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain {'Would undo' if o.dry_run else 'Undoing'} gain changes on {len(o.files)} file(s)")
            self.p()
        results, tally = [], [0, 0]
        for file in o.files:
            name = _name(file)
            if o.dry_run:
                if self.talk:
                    self.p(f"  ~ [DRY RUN] {name} (would undo)")
                r = _file_result(file, status="dry_run", dry_run=True)
            else:
                mtime = _mtime(file) if o.preserve_timestamp else None
                try:
                    frames = mp3gain.undo_gain(file)
                    if frames == 0:
                        if self.talk:
                            self.p(f"  . {name} (no changes to undo)")
                        r = _file_result(file, status="skipped", frames=0)
                    else:
                        _restore(file, mtime)
                        if self.talk:
                            self.p(f"  v {name} ({frames} frames restored)")
                        r = _file_result(file, status="success", frames=frames)
                except mp3gain.Mp3GainError as ex:
                    if self.talk:
                        self.e(f"  x {name} - {ex}")
                    r = _file_result(file, status="error", error=str(ex))
            _count(r, tally)
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        else:
            self._dry_run_notice()
        return 0

    # ---- -r / -e, src/main.rs:1213-1282 and 1937-2001 ------------------------------------------------------------------
    def cmd_track_gain(self) -> int:
        o = self.o
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain Analyzing and {'would apply' if o.dry_run else 'applying'} track gain to {len(o.files)} file(s)")
            self.p(self._target_line())
            if o.gain_modifier != 0:
                self.p(f"  Gain modifier: {o.gain_modifier:+d} steps")
            self.p()
        results, tally = [], [0, 0]
        for file in o.files:
            r = self.process_track_gain(file)
            _count(r, tally)
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        else:
            self._dry_run_notice()
        return 0

    def process_track_gain(self, file: Path) -> dict:
        o = self.o
        name = _name(file)
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"  -> {pre}Analyzing {name}...")
        try:
            rg = self.analyze_track(file)
        except rgmod.ReplayGainError as ex:
            if self.talk:
                self.e(f"  x {name} - {ex}")
            return _file_result(file, status="error", error=str(ex))
        base = rg.gain_steps()
        modified = base + o.gain_modifier
        if self.talk:
            extra = f" + {o.gain_modifier} = {modified}" if o.gain_modifier != 0 else ""
            self.p(f"      Loudness: {rg.loudness_db:.1f} dB, Gain: {rg.gain_db:+.1f} dB ({base} steps{extra}), Peak: {rg.peak:.4f}")
            if getattr(rg, "dynamics", None) is not None:
                self.p(f"      {_dyn_text(rg.dynamics)}")
        if modified == 0:
            if self.talk:
                self.p(f"  . {name} (no adjustment needed)")
            return _file_result(file, status="skipped", loudness_db=rg.loudness_db, loudness_lufs=_lufs(rg), **_dyn(rg), peak=rg.peak, gain_applied_steps=0,
                                gain_applied_db=0.0)
        return self.apply_replaygain(file, modified, rg, None)

    # ---- process_apply_replaygain_with_album, src/main.rs:2012-2170; AAC branch :2173-2241 -----------------------------
    def apply_replaygain(self, file: Path, steps: int, rg: rgmod.ReplayGainResult, album: Optional[Tuple[float, float]]) -> dict:
        o = self.o
        name = _name(file)
        pre = "[DRY RUN] " if o.dry_run else ""
        mtime = _mtime(file) if o.preserve_timestamp and not o.dry_run else None
        actual, warning = steps, None
        if steps > 0 and not o.wrap_gain:
            new_peak = rg.peak * 10.0 ** (rg.gain_db / 20.0)
            if new_peak > 1.0:
                if o.prevent_clipping:
                    actual = max(mp3gain.db_to_steps(-20.0 * math.log10(rg.peak)), 0)
                    if self.talk:
                        self.e(f"  ! {pre}{name} - gain reduced from {steps} to {actual} steps to prevent clipping (peak: {rg.peak:.4f})")
                    warning = f"gain reduced from {steps} to {actual} steps to prevent clipping (peak: {rg.peak:.4f})"
                elif not o.ignore_clipping and not o.quiet:
                    if self.text:
                        self.e(f"  ! {pre}{name} - clipping warning: peak would be {new_peak:.2f} (>{1.0:.2f})")
                        self.e("      Use -c to ignore clipping warnings or -k to prevent clipping")
                    warning = f"clipping warning: peak would be {new_peak:.2f} (>1.00)"
        is_aac = rg.file_type == rgmod.AudioFileType.Aac
        if o.dry_run:
            if self.talk:
                self.p(f"  ~ [DRY RUN] {name} (would apply {actual * GAIN_STEP_DB:+.1f} dB, {actual} steps{' (tags only)' if is_aac else ''})")
            return _file_result(file, status="dry_run", loudness_db=rg.loudness_db, loudness_lufs=_lufs(rg), **_dyn(rg), peak=rg.peak, gain_applied_steps=actual,
                                gain_applied_db=actual * GAIN_STEP_DB, warning=warning, dry_run=True)
        if is_aac:  # AAC samples cannot be changed losslessly: ReplayGain tags only
            tags = mp4meta.ReplayGainTags()
            tags.set_track(rg.gain_db, rg.peak)
            if album is not None:
                tags.set_album(*album)
            try:
                mp4meta.write_replaygain_tags(file, tags)
            except mp4meta.Mp4MetaError as ex:
                if self.talk:
                    self.e(f"  x {name} - {ex}")
                return _file_result(file, status="error", error=str(ex))
            _restore(file, mtime)
            if self.talk:
                self.p(f"  v {name} ({'track+album tags' if album is not None else 'tags'} written, {rg.gain_db:+.1f} dB)")
            return _file_result(file, status="success", loudness_db=rg.loudness_db, loudness_lufs=_lufs(rg), **_dyn(rg), peak=rg.peak, gain_applied_steps=rg.gain_steps(),
                                gain_applied_db=rg.gain_db, warning=warning)
        if _is_riff_wave(file):
            # The reference cannot get here (its probe knows no WAV); this library analyses WAV, but PCM has no global_gain
            # fields: the frame scanner would take false syncs in the samples for frames and rewrite audio bytes.
            msg = "RIFF/WAVE input is analysed only: lossless gain applies to MPEG Layer III frames"
            if self.talk:
                self.e(f"  x {name} - {msg}")
            return _file_result(file, status="error", error=msg)
        if _is_flac(file):
            # FLAC has no global_gain fields either; ReplayGain tags (Vorbis comments) are not written yet
            msg = "FLAC input is analysed only: lossless gain applies to MPEG Layer III frames"
            if self.talk:
                self.e(f"  x {name} - {msg}")
            return _file_result(file, status="error", error=msg)
        fn = mp3gain.apply_gain_with_undo_wrap if o.wrap_gain else mp3gain.apply_gain_with_undo
        try:
            frames = self._with_temp_file(file, lambda f: fn(f, actual))
        except (mp3gain.Mp3GainError, OSError) as ex:
            if self.talk:
                self.e(f"  x {name} - {ex}")
            return _file_result(file, status="error", error=str(ex))
        _restore(file, mtime)
        if self.talk:
            self.p(f"  v {name} ({frames} frames, {actual * GAIN_STEP_DB:+.1f} dB)")
        return _file_result(file, status="success", frames=frames, loudness_db=rg.loudness_db, loudness_lufs=_lufs(rg), **_dyn(rg), peak=rg.peak, gain_applied_steps=actual,
                            gain_applied_db=actual * GAIN_STEP_DB, warning=warning)

    # ---- -a, src/main.rs:1284-1452 -------------------------------------------------------------------------------------
    def cmd_album_gain(self) -> int:
        o = self.o
        pre = "[DRY RUN] " if o.dry_run else ""
        if self.talk:
            self.p(f"{pre}mp3rgain Analyzing album gain for {len(o.files)} file(s)")
            self.p(self._target_line())
            if o.gain_modifier != 0:
                self.p(f"  Gain modifier: {o.gain_modifier:+d} steps")
            self.p()
            self.p("  -> Analyzing tracks...")
        try:
            album = self._analyze_album_r128() if o.r128 else self.analyzer().analyze_album_files(o.files, o.track_index)
        except rgmod.ReplayGainError as ex:
            if o.output_format == "json":
                _print_json(self.out, summary=_summary(len(o.files), 0, len(o.files), o.dry_run))
            else:
                self.e(f"error: Failed to analyze album: {ex}")
            return 1
        base = album.album_gain_steps()
        steps = base + o.gain_modifier
        if self.talk:
            self.p()
            self.p(f"  Album loudness: {album.album_loudness_db:.1f} dB")
            extra = f" + {o.gain_modifier} = {steps}" if o.gain_modifier != 0 else ""
            self.p(f"  Album gain:     {album.album_gain_db:+.1f} dB ({base} steps{extra})")
            self.p(f"  Album peak:     {album.album_peak:.4f}")
            if getattr(album, "dynamics", None) is not None:
                self.p(f"  Album {_dyn_text(album.dynamics)}")
                for f, t in zip(o.files, album.tracks):
                    self.p(f"    {_name(f)}: {_dyn_text(t.dynamics)}")
            self.p()
        album_json = {"loudness_db": album.album_loudness_db, "gain_db": album.album_gain_db, "gain_steps": steps, "peak": album.album_peak}
        if _lufs(album) is not None:
            album_json["loudness_lufs"] = _lufs(album)
        album_json.update(_dyn(album))
        if steps == 0:
            if o.output_format == "json":
                files = [_file_result(f, status="skipped", loudness_db=t.loudness_db, loudness_lufs=_lufs(t), **_dyn(t), peak=t.peak, gain_applied_steps=0, gain_applied_db=0.0)
                         for f, t in zip(o.files, album.tracks)]
                _print_json(self.out, files=files, album=album_json, summary=_summary(len(o.files), 0, 0, o.dry_run))
            elif not o.quiet:
                self.p("  . No adjustment needed")
            return 0
        results, tally = [], [0, 0]
        for file, track in zip(o.files, album.tracks):
            r = self.apply_replaygain(file, steps, track, (album.album_gain_db, album.album_peak))
            _count(r, tally)
            if o.output_format == "json":
                results.append(r)
        if o.output_format == "json":
            _print_json(self.out, files=results, album=album_json, summary=_summary(len(o.files), tally[0], tally[1], o.dry_run))
        else:
            self._dry_run_notice()
        return 0


def _signed(x: float, prec: int) -> str:  # `{:+.N}`
    return "+inf" if math.isinf(x) and x > 0 else f"{x:+.{prec}f}"


def _plain(x: float, prec: int) -> str:  # `{:.N}`
    return "inf" if math.isinf(x) and x > 0 else f"{x:.{prec}f}"


def _mtime(file: Path):
    try:
        st = os.stat(file)
        return (st.st_atime_ns, st.st_mtime_ns)
    except OSError:
        return None


def _restore(file: Path, t):  # restore_timestamp, src/main.rs:2243-2247
    if t is not None:
        try:
            os.utime(file, ns=(os.stat(file).st_atime_ns, t[1]))
        except OSError:
            pass


def expand_files_recursive(paths: List[Path]) -> List[Path]:  # src/main.rs:436-470
    out: List[Path] = []

    def walk(d: Path):
        for entry in os.scandir(d):
            p = Path(entry.path)
            if entry.is_dir():
                walk(p)
            elif p.suffix.lower() in (".mp3", ".m4a", ".aac", ".mp4", ".flac"):
                out.append(p)

    for p in paths:
        if p.is_dir():
            walk(p)
        else:
            out.append(p)
    return sorted(out)


def print_version(out):  # src/main.rs:2254-2259
    print(f"mp3rgain_amd version {VERSION} (command-line compatible with mp3rgain 1.5.0)", file=out)
    print("MI355X-native ReplayGain analysis behind mp3rgain's interface", file=out)
    print(file=out)
    print(f"Each gain step = {_rust_float(GAIN_STEP_DB)} dB", file=out)


def print_usage(out):  # src/main.rs:2261-2346, shortened to the option table
    print(f"mp3rgain_amd version {VERSION}", file=out)
    print("Lossless MP3 volume adjustment and GPU ReplayGain analysis - mp3rgain's command line", file=out)
    print(file=out)
    print("USAGE:", file=out)
    print("    python -m mp3rgain_amd [OPTIONS] <FILES>...", file=out)
    print(file=out)
    print("OPTIONS:", file=out)
    for line in (
        f"-g <i>      Apply gain of i steps (each step = {_rust_float(GAIN_STEP_DB)} dB)",
        "-d <n>      Modify the suggested dB gain by n (TSV info output)",
        "-l <c> <g>  Apply gain to left (0) or right (1) channel only",
        "-m <i>      Modify suggested gain by integer i",
        "-r          Apply Track gain (ReplayGain analysis)",
        "-a          Apply Album gain (ReplayGain analysis)",
        "-e          Skip album analysis (even with multiple files)",
        "-i <n>      Specify which audio track to process (default: 0)",
        "-u          Undo gain changes (restore from APEv2 tag)",
        "-x          Only find max amplitude of file",
        "-s <mode>   Stored tag handling: c check, d delete, s skip, r recalc, i ID3v2, a APEv2",
        "-p          Preserve original file timestamp",
        "-c          Ignore clipping warnings",
        "-k          Prevent clipping (automatically limit gain)",
        "-w          Wrap gain values (instead of clamping)",
        "-t          Use temp file for writing",
        "-f          Assume MPEG 2 Layer III (compatibility, no effect)",
        "-q          Quiet mode (less output)",
        "-R          Process directories recursively",
        "-n          Dry-run mode (show what would be done)",
        "--dry-run   Same as -n",
        "-o <fmt>    Output format: 'text' (default), 'json', or 'tsv'",
        "--decoder <cmd>  Decoder command for files that are not WAV: writes a WAV stream to stdout, {} = file",
        "--r128      Analyse after EBU R 128 / ITU-R BS.1770 (ReplayGain 2.0: gain to -18 LUFS) instead of ReplayGain 1.0",
        "--true-peak With --r128: report and clip-limit on the true peak (4x / 2x oversampled)",
        "--range     With --r128: also report loudness range (EBU Tech 3342), maximum momentary and short-term loudness",
        "--surround  With --r128: weight every channel of a multichannel file by its layout (BS.1770: surrounds 1.41, LFE 0)",
        "--verify    Verify FLAC files: decode on the GPU and compare the PCM's MD5 with the signature in STREAMINFO",
        "            MP3 files: dropped frames, frame CRCs, and the LAME tag's music length, music CRC and tag CRC",
        "--rip       The files are the tracks of one ripped disc (16-bit stereo WAV or FLAC), in order: CRC-32, CRC-32 without",
        "            null samples and AccurateRip v1 / v2 signatures per track, computed on the GPU",
        "--rip-log <log>  With --rip: compare with the track sections of a ripper's log (EAC, XLD), in order",
        "--rip-offsets    With --rip --rip-log: AccurateRip signatures at every sample offset within +-2939 on the GPU, and the",
        "            offset at which the log's signatures match (another pressing, an uncorrected drive read offset)",
        "--stats     PCM defect scan on the GPU (WAV, FLAC, MP3): per channel peak, DC offset, clipped samples and clip runs, bits",
        "            in use, dropouts (zero runs inside the audio); per file the digital silence at its edges.  A report: exit",
        "            status 1 only for a file that fails or has dropped frames",
        "--clip-run <n>   With --stats: full-scale samples in a row that count as a clip run (default 3)",
        "--zero-run <n>   With --stats: zero samples in a row inside the audio that count as a dropout (default 64)",
        "--spectrum  Spectral scan on the GPU (WAV, FLAC, MP3): per channel the frequency above which there is nothing and the depth",
        "            of the edge there -- a lossless file made from a lossy one, a high-rate file made from a CD.  A report: exit",
        "            status 1 only for a file that fails or has dropped frames",
        "--edge-db <dB>   With --spectrum: how far the spectrum must fall across the edge (default 30)",
        "--min-cutoff <Hz>  With --spectrum: edges below this frequency are not reported (default 4000)",
        "--dr        Dynamic range (DR) on the GPU (WAV, FLAC, MP3): per file `DR<n>  peak dB  RMS dB  name`, per channel DR, peak,",
        "            RMS and the blocks that counted, and a closing `album DR` line for more than one file.  3-second blocks, RMS",
        "            with the factor 2, the loudest fifth of the blocks, the second-highest block peak: after the published",
        "            description of the TT DR meter, unverified against it.  JSON fields: dr, dr_mean, peak_db, rms_db, frames,",
        "            sample_rate, block_frames, dropped_frames, verdicts, channels[dr, peak_db, rms_db, top_ms, mean_square, peak,",
        "            peak2, blocks, top_blocks, nonfinite], album_dr.  Exit status 1 only for a file that fails or has dropped frames",
        "--dr-top <permille>  With --dr: the share of the loudest blocks that count (default 200)",
        "--ancestry  Lossy ancestry scan on the GPU (WAV, FLAC, MP3): is this PCM a decoded MP3?  The audio goes through the MP3",
        "            encoder's filterbank at all 576 alignments, per channel and, for stereo, mid and side; on the stream's granule",
        "            grid a large share of the lines falls to zero.  Per file `mp3 grid at +R (z, xISO[, mid/side])` or `no grid",
        "            found`, per view the numbers.  A convention of this project, tried on its own encoder's streams and held to no",
        "            other checker; not found: finely coded streams (a mono stream of 320 kb/s), short-block passages, AAC / Vorbis /",
        "            Opus, audio resampled or re-dithered after decoding.  JSON fields: mp3_grid, grid_offset, z, iso, midside,",
        "            best_view, segments, granules, dropped_frames, verdicts, views[view, offset, ratio, second, p0, z, iso, small,",
        "            active, active_total, flagged, nonfinite].  Exit status 1 only for a file that fails or has dropped frames",
        "--ancestry-segments <S>  With --ancestry: segments per file, spread evenly (default 16; 0 = the whole file)",
        "--ancestry-granules <G>  With --ancestry: granules of 576 samples per segment (default 32)",
        "--duplicates  Which of these files are the same recording?  On the GPU (WAV, FLAC, MP3): a sub-band-difference fingerprint",
        "            per file (a 32-bit code per 512 samples, 33 bands from 300 to 2000 Hz), then every pair of files at every offset",
        "            within the radius, by the share of differing bits.  Finds the same audio after lossy coding, a gain change, some",
        "            samples of delay or silence in front; not across sample rates, not from 96 kHz up, not time-stretched or",
        "            pitch-shifted copies, not excerpts offset by more than the radius.  A paragraph per group of more than one file",
        "            (offset and differing bits against its first file) and `N files, G groups of duplicates`.  A convention of this",
        "            project, compatible with no other fingerprint; the threshold was measured on synthetic material only.  JSON:",
        "            files[group, matches, codes, verdicts, ...], pairs[i, j, lag_codes, lag_seconds, errors, bits, ber], groups.",
        "            Exit status 1 only for a file that fails or has dropped frames",
        "--dup-radius <seconds>  With --duplicates: the largest offset looked for (default 5.94 = 512 codes at 44.1 kHz; at most 23.7)",
        "--dup-any-rate  With --duplicates: every file is brought to 11025 Hz on the GPU first, so the 44.1 kHz rip and the 48 / 96 / 192 kHz",
        "            download of the same master match; each member is shown with its own sample rate.  --dup-radius then defaults to",
        f"            5.94 s = 128 codes of 46.4 ms, --dup-ber to {_capi.XR_MAX_BER_PERMILLE}",
        "--dup-ber <permille>  With --duplicates: the share of differing bits up to which a pair matches (default 316)",
        "--tempo     How fast is each file?  On the GPU (WAV, FLAC, MP3): an onset curve (one value per 512 samples from 32 bands between",
        "            60 and 8000 Hz), its autocorrelation over windows of 1024 onsets, and a constant-tempo beat grid.  A line per file:",
        "            `128.00 BPM  (confidence 0.89, steady 1.00, first beat 0.157 s)  name`, or `no tempo found`.  The reading lies in",
        "            [--tempo-min, twice that): the octave is a convention.  `steady` is the share of windows that agree with the",
        "            file's tempo; the first beat is coarse (a 93 ms window).  A convention of this project, tried on synthetic",
        "            material only and held to no other BPM tool.  JSON: files[bpm, confidence, steady, first_beat_seconds, period16,",
        "            verdicts, ...].  Exit status 1 only for a file that fails or has dropped frames",
        "--tempo-min <BPM>  With --tempo: the lowest tempo reported (default 80; 30 to 300)",
        "--key       In which musical key is each file?  On the GPU (WAV, FLAC, MP3): the signal decimated to 5 .. 10 kHz, a chroma row per",
        "            512 decimated samples from 60 semitone bands (C2 .. B6, A4 = 440 Hz), the rows summed and matched against the",
        "            Krumhansl-Kessler profiles of the 24 keys.  A line per file: `A minor  (8A, correlation 0.93, margin 0.27, steady",
        "            1.00)  name`, or `no key found`: the Camelot code, the correlation with the profile, the lead over the runner-up, and",
        "            the share of segments that agree.  A convention of this project, tried on synthetic material only and held to no",
        "            other key finder.  JSON: files[key, camelot, open_key, correlation, margin, steady, verdicts, ...].  Exit status 1",
        "            only for a file that fails or has dropped frames",
        "--key-segment <rows>  With --key: the rows of a segment of `steady` (default 128, about 12 s; 8 to 4096)",
        "--stereo    How do the two channels of each file relate?  On the GPU (WAV, FLAC, MP3): the exact moments of channels 0 and 1,",
        "            how many frames are equal, opposite or zero, and the cross-correlation of the channels at every delay within the",
        "            radius.  A line per file: `stereo  (correlation 0.62, side -7.1 dB, balance +0.3 dB)  name`, `dual mono`, `right",
        "            channel is the inverted left`, `right channel late by 3 samples (correlation 0.998 there, 0.41 in place)`,",
        "            `channels out of phase`, `one-sided`, `near mono`, `mono file`.  A convention of this project, tried on synthetic",
        "            material only and held to no other tool.  JSON carries every field of the record.  Exit status 1 only for a file",
        "            that fails or has dropped frames",
        "--compare   A null test: every FILE held against the first (the reference copy).  On the GPU (WAV, FLAC, MP3): the copies lined up",
        "            to the sample, one gain fitted, what is left sized per second.  A line per file: `identical  name`, `identical samples,",
        "            starts 588 samples later  name`, `same master  (gain -3.01 dB, residual 0.31 LSB^2)  name`, `same recording, differs",
        "            (null -23.4 dB after +0.2 dB, worst 1:02-1:03 at -9.1 dB, first difference at 0:00.013)  name`, `not the same recording`.",
        "            A convention of this project, held to no other tool; exit status 1 only for a failing file or dropped frames",
        "--compare-radius <N>  With --compare: how far from the coarse lag the fine lag is looked for, in samples (default 1024; 0 to 2047)",
        "--compare-hint <FRAMES>  With --compare: the expected lag of every file, instead of the fingerprint match",
        "--stereo-radius <N>  With --stereo: the largest delay looked for, in samples (default 64; 0 to 255)",
        "--encode    Encode the files (WAV with 8, 16 or 24-bit integer samples, FLAC) to FLAC on the GPU, into <--encode-dir>/<stem>.flac:",
        "            LPC search at every even order, exact Rice sizing of every candidate, mid/side for two channels.  Unless",
        "            --no-encode-verify each stream is decoded again on the GPU and its MD5 held to the source's before its file is",
        "            written.  An output that exists is never replaced.  A FLAC source keeps its tags and pictures; no SEEKTABLE is",
        "            written.  Float WAV and MP3 sources are refused.  Exit status 1 for any failing file",
        "--encode-dir <DIR>  With --encode (required): where the outputs go",
        "--encode-lpc <N>  With --encode: the largest LPC order tried (default 8; 0 to 12, 0 = FIXED predictors only)",
        "--encode-block <N>  With --encode: the block size (default 4096; 256, 512, 1024, 2048 or 4096)",
        "--no-encode-verify  With --encode: write without decoding the streams again",
        "--clicks    Are there clicks or glitches in each file?  On the GPU (WAV, FLAC, MP3): every channel is predicted block by block by",
        "            the FLAC encoder's linear model, and a sample whose prediction error stands far above the median error around it is",
        "            flagged; flagged samples close together make an event, a narrow event is a click, a wide one a burst.  A line per",
        "            file: `no clicks  name`, `3 clicks (first at 1:02.345 left, strongest x41.2 at 2:10.007 right), 1 burst  name`, and",
        "            under it the first events, one per line.  A convention of this project, tried on synthetic material only and held",
        "            to no other tool.  JSON carries every field of the record.  Exit status 1 only for a file that fails or has dropped",
        "            frames",
        "--click-ratio <X>  With --clicks: how many times the local median a residual has to be (default 8.371, measured on synthetic",
        "            material; 1 to 1000)",
        "--click-order <P>  With --clicks: the predictor's order (default 8; even, 2 to 12)",
        "--click-block <B>  With --clicks: the samples of a block (default 1024; 256, 512, 1024, 2048 or 4096)",
        "--click-list <K>  With --clicks: how many events are listed per file (default 16; 0 to 256)",
        "-v          Show version",
        "-h          Show this help",
    ):
        print("    " + line, file=out)
    print(file=out)
    print("NOTES:", file=out)
    print(f"    - Each gain step = {_rust_float(GAIN_STEP_DB)} dB (fixed by MP3 specification)", file=out)
    print("    - Changes are lossless and reversible; gain changes are stored in APEv2 tags for undo support", file=out)
    print(f"    - ReplayGain analysis runs on the GPU (target: {_rust_float(REFERENCE_DB)} dB); there is no CPU path", file=out)


def main(argv: Optional[List[str]] = None, out=None, err=None) -> int:
    """main, src/main.rs:171-181."""
    out = out or sys.stdout
    err = err or sys.stderr
    args = list(sys.argv[1:] if argv is None else argv)
    if not args:
        print_usage(out)
        return 0
    try:
        opts = parse_args(args, out, err)
        return Cli(opts, out, err).run()
    except Exit as ex:
        return ex.code
    except CliError as ex:
        print(f"Error: {ex}", file=err)
        return 1
