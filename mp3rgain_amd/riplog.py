"""A small reader of CD ripper logs, so that the numbers of `Analyzer.rip_checksums` can be compared with what a ripper wrote.

PROVENANCE: the line shapes below are written from memory of EAC and XLD logs.  No real rip log was at hand when this module
was written or tested; the tests hold it to logs they write themselves in both shapes.

What is read:
  * bytes that begin with a UTF-16 byte-order mark decode as UTF-16 (EAC writes UTF-16 LE), anything else as UTF-8 with
    replacement characters;
  * a track section starts at a line that is `Track` followed by a number and nothing else (`Track  1`, `Track 01`) and runs
    to the next such line;
  * inside a section, the first word of 8 hexadecimal digits is taken from the first line containing each of
        Copy CRC                     (EAC)  -> copy_crc
        CRC32 hash (skip zero)       (XLD)  -> crc32_skip_zero
        CRC32 hash                   (XLD)  -> crc32
        AccurateRip v1 signature     (XLD)  -> arv1
        AccurateRip v2 signature     (XLD)  -> arv2
Anything else is ignored.  A log does not say whether EAC's "Copy CRC" was taken with null samples or without, so it matches
when it equals either CRC.

`find_offset` answers a log written from another pressing, or by a drive whose read offset was not corrected: with the
signatures of `Analyzer.rip_offset_signatures` it looks for the one sample offset at which every logged AccurateRip signature
is the computed one."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

_TRACK = re.compile(r"^Track\s*(\d+)$")
_HEX8 = re.compile(r"(?<![0-9A-Za-z])[0-9A-Fa-f]{8}(?![0-9A-Za-z])")
# (text the line contains, field); the longer of two texts that share a beginning comes first
_KEYS = (("Copy CRC", "copy_crc"), ("CRC32 hash (skip zero)", "crc32_skip_zero"), ("CRC32 hash", "crc32"),
         ("AccurateRip v1 signature", "arv1"), ("AccurateRip v2 signature", "arv2"))


@dataclass
class LogTrack:
    """One track section of a log: the values it holds, None for those it does not."""
    number: int
    copy_crc: Optional[int] = None
    crc32: Optional[int] = None
    crc32_skip_zero: Optional[int] = None
    arv1: Optional[int] = None
    arv2: Optional[int] = None


@dataclass
class Verdict:
    """A track's log section against its computed checksums.  `checks`: (name, logged, [computed values it may equal], ok).
    With an `offset` other than 0 (compare_at) the AccurateRip values are those at that offset, and a CRC check's `ok` is None:
    the log's CRC is over other samples, so it says nothing either way."""
    ok: bool
    checks: List[Tuple[str, int, List[int], Optional[bool]]] = field(default_factory=list)
    offset: int = 0

    @property
    def text(self) -> str:
        if not self.checks:
            return "nothing to compare"
        bad = [name for name, _, _, ok in self.checks if ok is False]
        if not self.offset:
            return "mismatch: " + ", ".join(bad) if bad else "match"
        parts = []
        if bad:
            parts.append("mismatch: " + ", ".join(bad))
        elif any(ok for _, _, _, ok in self.checks):
            parts.append(f"match at offset {self.offset:+d}")
        if any(ok is None for _, _, _, ok in self.checks):
            parts.append(f"CRC-32 not comparable at offset {self.offset:+d}")
        return "; ".join(parts)

    def check_text(self, ok: Optional[bool]) -> str:
        if ok is None:
            return f"not comparable at offset {self.offset:+d}"
        if not ok:
            return "mismatch"
        return f"match at offset {self.offset:+d}" if self.offset else "match"


def compare_at(log: LogTrack, offset: int, arv1: int, arv2: int) -> Verdict:
    """The section against the AccurateRip signatures `arv1`, `arv2` computed at the sample offset `offset` != 0."""
    checks = []
    for name, logged in (("Copy CRC", log.copy_crc), ("CRC32 hash", log.crc32), ("CRC32 hash (skip zero)", log.crc32_skip_zero)):
        if logged is not None:
            checks.append((name, logged, [], None))
    for name, logged, value in (("AccurateRip v1", log.arv1, arv1), ("AccurateRip v2", log.arv2, arv2)):
        if logged is not None:
            checks.append((name, logged, [value], logged == value))
    return Verdict(all(ok is not False for _, _, _, ok in checks), checks, offset)


@dataclass
class OffsetSearch:
    """What find_offset found.  `offset`: the common offset, or None; `tracks` / `signatures`: how many log sections and how
    many logged AccurateRip signatures took part."""
    offset: Optional[int]
    tracks: int
    signatures: int

    @property
    def text(self) -> str:
        if not self.signatures:
            return "nothing to compare"
        if self.offset is None:
            return f"no common offset for {self.signatures} signature(s) of {self.tracks} track(s)"
        return f"offset {self.offset:+d} matches {self.signatures} signature(s) of {self.tracks} track(s)"


def decode(data: bytes) -> str:
    if data[:2] in (b"\xff\xfe", b"\xfe\xff"):
        return data.decode("utf-16", "replace")
    return data.decode("utf-8", "replace")


def parse(data: bytes) -> List[LogTrack]:
    """The track sections of a log, in the order they appear."""
    tracks: List[LogTrack] = []
    cur: Optional[LogTrack] = None
    for line in decode(data).splitlines():
        line = line.strip().lstrip("\ufeff")
        m = _TRACK.match(line)
        if m:
            cur = LogTrack(int(m.group(1)))
            tracks.append(cur)
            continue
        if cur is None:
            continue
        for text, name in _KEYS:
            if text in line:
                h = _HEX8.search(line)
                if h and getattr(cur, name) is None:
                    setattr(cur, name, int(h.group(0), 16))
                break
    return tracks


def compare(log: LogTrack, sums) -> Verdict:
    """`sums`: anything with crc32, crc32_nonnull, arv1 and arv2 (replaygain.RipChecksums)."""
    checks = []
    for name, logged, may in (("Copy CRC", log.copy_crc, [sums.crc32, sums.crc32_nonnull]),
                              ("CRC32 hash", log.crc32, [sums.crc32]),
                              ("CRC32 hash (skip zero)", log.crc32_skip_zero, [sums.crc32_nonnull]),
                              ("AccurateRip v1", log.arv1, [sums.arv1]),
                              ("AccurateRip v2", log.arv2, [sums.arv2])):
        if logged is not None:
            checks.append((name, logged, may, logged in may))
    return Verdict(all(ok for _, _, _, ok in checks), checks)


def find_offset(sections: List[LogTrack], offsets) -> OffsetSearch:
    """`offsets`: anything with radius and arv1 / arv2 as [n][2 radius + 1] tables, [t][o + radius]
    (replaygain.RipOffsetSignatures); section t is track t.  For every section that holds arv1 or arv2, the offsets at which
    each logged signature equals the table; the sets are intersected over all such tracks and both versions, and the common
    offset with the smallest |o| is the answer (the negative one on a tie).  A track that matches everywhere -- all zeros --
    constrains nothing.  Sections beyond the table's tracks take no part."""
    radius = int(offsets.radius)
    common = None  # None = every offset so far
    tracks = signatures = 0
    for t, sec in enumerate(sections[:len(offsets.arv1)]):
        took_part = False
        for logged, row in ((sec.arv1, offsets.arv1[t]), (sec.arv2, offsets.arv2[t])):
            if logged is None:
                continue
            took_part = True
            signatures += 1
            here = {k - radius for k in range(2 * radius + 1) if int(row[k]) == logged}
            common = here if common is None else common & here
        tracks += took_part
    if not signatures or not common:
        return OffsetSearch(None, tracks, signatures)
    return OffsetSearch(min(common, key=lambda o: (abs(o), o)), tracks, signatures)
