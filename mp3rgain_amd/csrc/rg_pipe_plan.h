// rg_pipe_plan.h -- the two sizing rules of the MP3 loader pipeline (rg_mp3_pipe.hip), free of HIP so that a host compiler
// alone can exercise them (tests/test_pipe_plan_cpu.py): how many granule-channels the open chunk may hold, and whether a
// decoded chunk's tracks are analysed right away as an album part.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

// Granule-channels per chunk.  The Huffman kernel deals a chunk's units to its lanes heaviest first (rg_mp3_sort_*): a chunk
// has to be several generations of its blocks (256 CUs x 2 blocks x 512 threads = 262144 resident) for the light tail to fill
// in behind the heavy head, and the six small launches in front of it (frame parser, sort) are paid per chunk: per 256 K units
// the chain takes 0.68 / 0.63 / 0.56 / 0.56 ms in chunks of 256 K / 384 K / 768 K / 1 M on the dense 320 kb/s stream.
constexpr uint64_t kPipeChunkUnits = 786432;

// The most units chunk `open_index` of a call may hold; `chunk_units` are in it already, `files_placed` of the call's `n_files`
// files have their place in a chunk, with `units_placed` units between them.  *tapering is set (never cleared) when the taper
// is what limits the chunk.
inline uint64_t rg_pipe_unit_cap(size_t open_index, uint64_t chunk_units, bool starved, size_t files_placed, uint64_t units_placed,
                                 size_t n_files, bool *tapering) {
    // (the call's first chunks are smaller: the device has nothing to do until the first one is complete)
    uint64_t unit_cap = open_index < 3 ? kPipeChunkUnits >> (3 - open_index) : kPipeChunkUnits;  // 1/8, 1/4, 1/2, then whole chunks
    // ... and where the device waits for the loaders, the call's last chunks the other way round (each at most
    // half of what is left, by the files so far): what follows the last file is one chunk's copy, decode and
    // analysis, 3.5 ms of a 26 ms call for a whole chunk (two loader threads, 256 VBR files)
    if (starved && files_placed) {
        const uint64_t left = chunk_units + (uint64_t)((double)(n_files - files_placed) * ((double)units_placed / (double)files_placed));
        const uint64_t taper = std::max(left / 2, kPipeChunkUnits >> 3);
        if (taper < unit_cap) {
            unit_cap = taper;
            *tapering = true;  // (small chunks follow each other quickly: the device being busy then says nothing)
        }
    }
    return unit_cap;
}

// A chunk whose H2D copy takes longer than its decode leaves the device idle: its tracks (and what is pending) become a part
// right away.  Where the decode is the longer stage a part only splits the analysis into smaller, less efficient launches
// (measured: 256 VBR files 20.6 -> 21.6 ms, 256 files of 320 kb/s 50.7 -> 38.4 ms), so such chunks wait -- for a later chunk
// that is copy-bound, or for the end of the album, where an album without a single part goes the plain way.
// Copy: ~50 GB/s; decode: ~0.5 ms per 256 K units = 1.9 ns per unit = 95 bytes' worth of copy.  At 104 bytes per unit (128 kb/s
// stereo) the two routes measure the same within their noise (album 24.9 -> 23.4 ms, track mode 21.6 -> 22.5), so the line is
// drawn at 120: 160 kb/s and up.
// (rg_ctx::parts_min_bpu(): RG_PARTS_MIN_BYTES_PER_UNIT as read at rg_create, or tuning key 11)
// `starved`: the device had finished the chunk's decode before the next chunk was ready -- the analysis then costs nothing.
inline bool rg_pipe_chunk_is_part(size_t used_bytes, uint64_t units, double min_bytes_per_unit, bool starved) {
    return (units && (double)used_bytes / (double)units >= min_bytes_per_unit) || starved;
}
