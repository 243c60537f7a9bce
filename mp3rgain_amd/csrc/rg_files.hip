// rg_files.hip -- the file-level entry points of the path (last row): analyze_track /
// analyze_album / find_peak_amplitude on files, as the reference's public functions take them
// (src/replaygain.rs:929-941, 1033-1074, 1140-1249).
//
// The reference gets PCM from symphonia (src/replaygain.rs:807-904).  Here a file is, by content:
//   * an MPEG-1/2/2.5 Layer III stream (optionally behind an ID3v2 tag): decoded by the library's own decoder
//     (rg_mp3dec.cpp, include/mp3rgain_amd_dec.h) into planar f32 that goes to HBM as it is -- the files of an
//     album are decoded on all host cores at once;
//   * a RIFF/WAVE file (integer PCM 8/16/24/32 bit, IEEE float 32 bit, plain or WAVE_FORMAT_EXTENSIBLE): the
//     interleaved bytes are copied to HBM and turned into the planar arena by a device kernel;
//   * anything else (M4A/AAC: no AAC decoder is built yet) through an external decoder command that writes a WAV
//     stream to stdout (rg_set_decoder_command, e.g. "ffmpeg -v error -i {} -f wav -c:a pcm_f32le -").
// Everything after the arena is the same path as rg_analyze_pcm_batch.
//
// This file holds the C entry points and their group helpers; the rest of the file layer: rg_wav.hip, rg_file_load.hip,
// rg_file_stage.hip, rg_mp3_pipe.hip, rg_file_hooks.hip (shared declarations: rg_files.h).
#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>

#include "rg_albums.h"
#include "rg_files.h"
#include "rg_flac_md5.h"
#include "rg_mp3verify.h"
#include "rg_r128.h"
#include "rg_rip.h"

using namespace rgf;

// One file, loaded and laid into the arena: *desc describes it, *file_type (if given) is what detect_file_type makes of it.
// Some(idx) selects among the audio tracks of a container (src/replaygain.rs:838-851); a WAV stream has one
static int load_and_stage_one(rg_ctx *c, const char *path, int32_t track_index, rg_track_desc *desc, size_t *arena_bytes,
                              uint32_t *file_type = nullptr) {
    std::vector<LoadedAudio> &pool = file_pool(c, 1);
    c->file_track_index = track_index;
    int rc = load_one(c, path, &pool);
    c->file_track_index = -1;
    if (rc != RG_OK) return rc;
    if (track_index >= 0 && (uint32_t)track_index >= pool[0].n_audio_tracks)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "Track index %d out of range (file has %u audio track(s))", track_index, pool[0].n_audio_tracks);
    std::vector<rg_track_desc> descs;
    rc = stage_loaded(c, pool, 1, &descs, arena_bytes);
    if (rc == RG_ERR_FORMAT) return rg_set_err(c, RG_ERR_FORMAT, "Failed to probe format: %s", path);  // src/replaygain.rs:815-822
    if (rc != RG_OK) return rc;
    *desc = descs[0];
    if (file_type) *file_type = pool[0].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
    return RG_OK;
}

// Album parts (PartsRun) for a group of `n_files` files of a call of `n_groups` groups: the loader pipeline decodes them, nobody
// else's stream is involved, and RG_ALBUM_PARTS=0 / tuning key 10 = 1 (tests, measurements) has not turned them off.
// (with fewer than three pipeline slots -- tuning key 3 -- a part's enqueue would find its slot's pinned descriptors still
// being copied behind the decode just issued and the drive thread would sit that decode out: no parts then)
// *use: whether; if so every slot's stream has been waited for -- the parts use every slot's buffers on the decode's stream,
// nothing of an earlier batch may be in flight.
static int parts_allowed(rg_ctx *c, size_t n_files, size_t n_groups, bool *use) {
    *use = c->parts_on() && c->n_slots >= 3 && n_groups <= 1 && n_files > 0 && c->gpu_mp3_decode >= 3 && !c->user_attached;
    if (*use) RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
    return RG_OK;
}

// The files of a group that came through loading (`slot`: their indices in `in`, ascending) as one batch: the good files to the
// front of the pool (swap keeps every buffer alive for the next call), into the arena, through `run(descs, k, arena_bytes, res)`,
// and res[k] -> out[slot[k]].  The status is the staging's or the run's: what a failed batch means is the caller's to say.
template <typename Result, typename Run>
static int run_good_files(rg_ctx *c, std::vector<LoadedAudio> &in, const std::vector<size_t> &slot, Result *out, Run run) {
    for (size_t k = 0; k < slot.size(); ++k)
        if (slot[k] != k) std::swap(in[k], in[slot[k]]);
    std::vector<rg_track_desc> descs;
    size_t arena_bytes = 0;
    int rc = stage_loaded(c, in, slot.size(), &descs, &arena_bytes);
    if (rc != RG_OK) return rc;
    std::vector<Result> res(slot.size());
    rc = run(descs.data(), slot.size(), arena_bytes, res.data());
    if (rc != RG_OK) return rc;
    for (size_t k = 0; k < slot.size(); ++k) out[slot[k]] = res[k];
    return RG_OK;
}
// a failure of the batch itself (a WAV of a kind the library cannot stage, a device error): every file in it carries it
// (status_out: the group's; `first`: the group's first file in the call's numbering, which file_errors has)
static void fail_batch(rg_ctx *c, const std::vector<size_t> &slot, size_t first, int rc, int32_t *status_out) {
    for (size_t k = 0; k < slot.size(); ++k) {
        status_out[slot[k]] = rc;
        c->file_errors[first + slot[k]] = c->err;
    }
}

// =================================================================================================
extern "C" int rg_set_decoder_command(rg_ctx *c, const char *command_template) {
    if (!c) return RG_ERR_INVALID_ARG;
    c->decoder_cmd = command_template ? command_template : "";
    return RG_OK;
}

extern "C" int rg_analyze_wav_batch(rg_ctx *c, const void *const *wav, const size_t *wav_len, size_t n, int album,
                                    rg_track_result *out, rg_album_result *album_out) {
    if (!c) return RG_ERR_INVALID_ARG;
    if (n && (!wav || !wav_len)) return rg_set_err(c, RG_ERR_INVALID_ARG, "null input array");
    std::vector<rg_track_desc> descs;
    size_t arena_bytes = 0;
    int rc = stage_wavs(c, wav, wav_len, n, &descs, &arena_bytes);
    if (rc != RG_OK) return rc;
    // the planar arena is on the device: the rest is rg_analyze_pcm_batch / rg_analyze_album_pcm, exact pass included
    if (album) return rg_analyze_album_pcm(c, descs.data(), n, c->d_arena.p, arena_bytes, 1, out, album_out, nullptr);
    return rg_analyze_pcm_batch(c, descs.data(), n, c->d_arena.p, arena_bytes, 1, out, nullptr);
}

extern "C" int rg_analyze_track(rg_ctx *c, const char *path, int32_t track_index, rg_track_result *out) {
    if (!c || !out) return RG_ERR_INVALID_ARG;
    rg_track_desc desc;
    size_t arena_bytes = 0;
    uint32_t file_type = 0;
    int rc = load_and_stage_one(c, path, track_index, &desc, &arena_bytes, &file_type);
    if (rc != RG_OK) return rc;
    rc = rg_analyze_pcm_batch(c, &desc, 1, c->d_arena.p, arena_bytes, 1, out, nullptr);
    if (rc != RG_OK) return rc;
    out->file_type = file_type;
    return RG_OK;
}

// Files of a long list in groups whose PCM is estimated (24 bytes of planar f32 per byte of file: a 128 kb/s stereo MP3;
// denser files decode to less) to stay within a third of the free device memory, at most 64 GB.
static void file_groups(rg_ctx *c, const char *const *paths, size_t n, std::vector<std::pair<size_t, size_t>> *groups) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)48 << 30;
    size_t budget = std::min((size_t)64 << 30, (free_b + c->d_arena.cap) / 3);
    if (c->group_bytes()) budget = c->group_bytes();  // tests: small groups
    groups->clear();
    for (size_t first = 0; first < n;) {
        size_t last = first, est = 0;
        while (last < n) {
            struct stat st;
            const size_t sz = (paths[last] && stat(paths[last], &st) == 0 && st.st_size > 0) ? (size_t)st.st_size : 0;
            if (last > first && est + sz * 24 > budget) break;
            est += sz * 24;
            ++last;
        }
        groups->push_back(std::make_pair(first, last - first));
        first = last;
    }
}

// analyze_album_with_index (src/replaygain.rs:1044-1074) up to, not including, the album percentile: per-file results in
// input order on the host, the album's [histogram | peak] pack ready on the device (rg_album_finish reads it out; on a
// node with several GPUs rg_album_exchange comes first, rg_node.cpp).  The first failing file IN INPUT ORDER aborts
// the album (:1055) -- the files of a group are loaded together, so every file's outcome is looked at before anything is
// reported -- and *failed_index (if given) says which one it was.  An album whose PCM does not fit the device at once is
// analysed in parts and the parts' histograms and peaks are folded (u32 adds commute: the result does not depend on the
// partition).
extern "C" int rg_analyze_album_begin(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *tracks_out,
                                      size_t *failed_index) {
    if (failed_index) *failed_index = (size_t)-1;
    if (!c || (n && (!paths || !tracks_out))) return RG_ERR_INVALID_ARG;
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    const bool trace = c->trace_files;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto fail_at = [&](size_t i, int code) {
        if (failed_index) *failed_index = i;
        return code;
    };
    for (size_t g = 0; g < std::max<size_t>(groups.size(), 1); ++g) {
        const size_t first = groups.empty() ? 0 : groups[g].first, cnt = groups.empty() ? 0 : groups[g].second;
        std::vector<LoadedAudio> &in = file_pool(c, cnt);
        const double t0 = now();
        std::vector<int> rcs;
        std::vector<std::string> errs;
        PartsRun parts;  // album parts: one album that fits the device
        bool use_parts = false;
        rc = parts_allowed(c, cnt, groups.size(), &use_parts);
        if (rc != RG_OK) return rc;
        c->file_track_index = track_index;
        rc = load_many(c, paths + first, cnt, &in, &rcs, &errs, use_parts ? &parts : nullptr);
        c->file_track_index = -1;
        if (rc != RG_OK) return rc;  // not a file's failure: *failed_index stays (size_t)-1, so that a node prefers real file errors of other shares
        for (size_t i = 0; i < cnt; ++i) {
            std::string msg;
            const int frc = file_outcome(in[i], rcs[i], errs[i], paths[first + i], track_index, &msg);
            if (frc != RG_OK) return fail_at(first + i, rg_set_err(c, frc, "%s", msg.c_str()));
        }
        const double t1 = now();
        if (use_parts && !parts.broken && parts.file_of.size() == cnt) {
            // every file was analysed as a part of its chunk: the results are on their way to the host, the packs are on the device
            RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
            bool flagged = false;
            for (size_t j = 0; j < cnt; ++j) {
                const rg_track_result &r = c->h_part_results.p[j];
                flagged = flagged || (c->kernel_variant == 0 && (r.flags & RG_TRACK_FLAG_IMPRECISE));
                tracks_out[first + parts.file_of[j]] = r;
            }
            if (!flagged) {  // (a flagged track: the plain route below repeats it on the order-faithful kernel)
                rc = rg_album_parts_fold(c, parts.n_parts);
                if (rc != RG_OK) return rc;
                for (size_t i = 0; i < cnt; ++i) tracks_out[first + i].file_type = in[i].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
                if (trace) fprintf(stderr, "[rg_analyze_album] load + decode + analysis in %zu parts %.1f ms, results %.1f ms\n", parts.n_parts, (t1 - t0) * 1e3, (now() - t1) * 1e3);
                return RG_OK;
            }
        }
        std::vector<rg_track_desc> descs;
        size_t arena_bytes = 0;
        rc = stage_loaded(c, in, cnt, &descs, &arena_bytes);
        if (trace) fprintf(stderr, "[rg_analyze_album] load %.1f ms, stage + device decode %.1f ms\n", (t1 - t0) * 1e3, (now() - t1) * 1e3);
        if (rc == RG_ERR_FORMAT) {  // "input i ..." -> the reference's text with the file's name
            size_t i = 0;
            if (sscanf(c->err.c_str(), "input %zu", &i) == 1 && i < cnt)
                return fail_at(first + i, rg_set_err(c, RG_ERR_FORMAT, "Failed to probe format: %s", paths[first + i]));
        }
        if (rc != RG_OK) return rc;  // not a file's failure: *failed_index stays (size_t)-1, so that a node prefers real file errors of other shares
        const double t2 = now();
        if (groups.size() <= 1) rc = rg_album_local_pcm(c, descs.data(), cnt, c->d_arena.p, arena_bytes, 1, tracks_out);
        else rc = rg_album_part(c, descs.data(), cnt, c->d_arena.p, arena_bytes, g, groups.size(), tracks_out + first);
        if (rc != RG_OK) return rc;  // not a file's failure: *failed_index stays (size_t)-1, so that a node prefers real file errors of other shares
        for (size_t i = 0; i < cnt; ++i) tracks_out[first + i].file_type = in[i].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
        if (trace) fprintf(stderr, "[rg_analyze_album] analysis %.1f ms\n", (now() - t2) * 1e3);
    }
    if (groups.size() > 1) return rg_album_parts_fold(c, groups.size());
    return RG_OK;
}

extern "C" int rg_analyze_album(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *tracks_out,
                                rg_album_result *album_out) {
    if (!c || (n && (!paths || !tracks_out)) || !album_out) return RG_ERR_INVALID_ARG;
    const int rc = rg_analyze_album_begin(c, paths, n, track_index, tracks_out, nullptr);
    if (rc != RG_OK) return rc;
    return rg_album_finish(c, album_out, nullptr);
}

// one group of rg_analyze_tracks: files [first, first + n) of the call; file_errors is indexed by the call's numbering
// (fold: rg_analyze_albums -- every batch's tracks are folded into their albums' packs as well)
static int analyze_tracks_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, int32_t track_index, rg_track_result *out,
                                int32_t *status_out, AlbumFold *fold = nullptr) {
    paths += first;
    out += first;
    status_out += first;
    std::vector<LoadedAudio> &in = file_pool(c, n);
    std::vector<int> rcs;
    std::vector<std::string> errs;
    // parts (PartsRun), track mode: every file of the group has to come through the loader pipeline for them to count
    PartsRun parts;
    parts.album = 0;
    parts.fold = fold;
    bool use_parts = false;
    int rc = parts_allowed(c, n, 1 /* the call's other groups do not matter: tracks are independent */, &use_parts);
    if (rc != RG_OK) return rc;
    c->file_track_index = track_index;
    rc = load_many(c, paths, n, &in, &rcs, &errs, use_parts ? &parts : nullptr);
    c->file_track_index = -1;
    if (rc != RG_OK) return rc;
    if (use_parts && !parts.broken && parts.file_of.size() == n) {
        RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
        bool flagged = false;
        for (size_t j = 0; j < n; ++j) flagged = flagged || (c->kernel_variant == 0 && (c->h_part_results.p[j].flags & RG_TRACK_FLAG_IMPRECISE));
        if (!flagged) {  // (else: the plain route below, which repeats flagged tracks on the order-faithful kernel)
            for (size_t j = 0; j < n; ++j) {
                const size_t i = parts.file_of[j];
                out[i] = c->h_part_results.p[j];
                out[i].file_type = in[i].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
                status_out[i] = RG_OK;
                c->file_errors[first + i].clear();
            }
            return RG_OK;
        }
    }
    if (fold && parts.n_parts) {  // parts were folded already: the plain route below starts the packs over
        rc = fold_init(c, fold);
        if (rc != RG_OK) return rc;
    }
    // the batch holds the files that loaded and whose rate the analysis knows; `slot` maps them back
    std::vector<size_t> slot;
    for (size_t i = 0; i < n; ++i) {
        memset(&out[i], 0, sizeof out[i]);
        status_out[i] = rcs[i];
        c->file_errors[first + i] = errs[i];
        if (rcs[i] != RG_OK) continue;
        std::string msg;
        const int frc = file_outcome(in[i], RG_OK, errs[i], paths[i], track_index, &msg);
        if (frc != RG_OK) {
            status_out[i] = frc;
            c->file_errors[first + i] = msg;
            continue;
        }
        if (fold && !stageable(in[i])) {  // rg_analyze_albums: this file fails alone instead of failing every file of the batch
            status_out[i] = RG_ERR_FORMAT;
            c->file_errors[first + i] = std::string("Failed to probe format: ") + paths[i];
            continue;
        }
        slot.push_back(i);
    }
    if (slot.empty()) return RG_OK;
    rc = run_good_files(c, in, slot, out, [&](const rg_track_desc *descs, size_t k, size_t arena_bytes, rg_track_result *res) {
        return rg_analyze_pcm_batch(c, descs, k, c->d_arena.p, arena_bytes, 1, res, nullptr);
    });
    if (rc != RG_OK) {
        fail_batch(c, slot, first, rc, status_out);
        return RG_OK;
    }
    for (size_t k = 0; k < slot.size(); ++k) out[slot[k]].file_type = in[k].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
    if (fold) return fold_batch(c, fold, slot.data(), slot.size(), c->slot().stream);
    return RG_OK;
}

// `-r` over a whole library must not need the whole library's PCM in HBM at once: the files are taken in groups
// (file_groups).  Tracks are independent, so the groups are too.
extern "C" int rg_analyze_tracks(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *out,
                                 int32_t *status_out) {
    if (!c || (n && (!paths || !out || !status_out))) return RG_ERR_INVALID_ARG;
    c->file_errors.assign(n, std::string());
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    for (const auto &g : groups) {
        rc = analyze_tracks_group(c, paths, g.first, g.second, track_index, out, status_out);
        if (rc != RG_OK) return rc;
    }
    return RG_OK;
}

extern "C" const char *rg_tracks_error(const rg_ctx *c, size_t i) {
    if (!c || i >= c->file_errors.size()) return "";
    return c->file_errors[i].c_str();
}

int rg_albums_check(const size_t *album_first, size_t n_albums, size_t n, std::string *msg) {
    char m[160];
    if (!album_first) {
        if (n_albums == 0 && n == 0) return RG_OK;
        *msg = "album_first is NULL";
        return RG_ERR_INVALID_ARG;
    }
    if (album_first[0] != 0) {
        snprintf(m, sizeof m, "album_first[0] is %zu, not 0", album_first[0]);
        *msg = m;
        return RG_ERR_INVALID_ARG;
    }
    if (album_first[n_albums] != n) {
        snprintf(m, sizeof m, "album_first[%zu] is %zu, not the number of files (%zu)", n_albums, album_first[n_albums], n);
        *msg = m;
        return RG_ERR_INVALID_ARG;
    }
    for (size_t a = 0; a < n_albums; ++a)
        if (album_first[a + 1] < album_first[a]) {
            snprintf(m, sizeof m, "album_first decreases from entry %zu to entry %zu", a, a + 1);
            *msg = m;
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

// Many albums in one call: rg_analyze_tracks' groups, loader pipeline and parts over the whole list, so that the pipeline
// stays full across album boundaries, with every batch's track histograms and peaks folded into their albums' live packs on
// the device (rg_albums.hip).  Only albums with files in the current group have a live pack.  An album is finished when the
// group that holds its last file is: its pack is read out with the others finished there (one launch, one copy back per
// group).  An album that goes on into the next group is carried in the pack in front of the live ones.  Per album the first
// failing file in input order decides (src/replaygain.rs:1055).  *files_done: the files whose outcome is final (the groups
// before the one in progress); done[a]: album a's record is final.
static int analyze_albums_impl(rg_ctx *c, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                               int32_t track_index, rg_track_result *tracks_out, int32_t *status_out, rg_album_result *albums_out,
                               int32_t *album_status_out, std::vector<char> &done, size_t *files_done) {
    std::vector<size_t> album_of(n);
    for (size_t a = 0; a < n_albums; ++a)
        for (size_t i = album_first[a]; i < album_first[a + 1]; ++i) album_of[i] = a;
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    // live packs: the albums that have files in one group (never more than its files), plus the carried pack in front of them
    size_t max_packs = 1, max_files = 1;
    for (const auto &g : groups) {
        size_t albums = 0;
        for (size_t i = g.first; i < g.first + g.second; ++i) albums += (i == g.first || album_of[i] != album_of[i - 1]) ? 1 : 0;
        max_packs = std::max(max_packs, albums);
        max_files = std::max(max_files, g.second);
    }
    RG_HIP(c, c->d_albums_packs.reserve((max_packs + 1) * (size_t)RG_ALBUMS_PACK_STRIDE));
    RG_HIP(c, c->d_albums_map.reserve(2 * max_files));  // a group's parts, and the plain route after them
    RG_HIP(c, c->h_albums_map.reserve(2 * max_files));
    RG_HIP(c, c->d_albums_res.reserve(max_packs));
    RG_HIP(c, c->h_albums_res.reserve(max_packs));
    uint32_t *const carry = c->d_albums_packs.p;
    hipStream_t s = c->slots[0].stream;
    auto album_status = [&](size_t a) -> int32_t {
        for (size_t i = album_first[a]; i < album_first[a + 1]; ++i)
            if (status_out[i] != RG_OK) return status_out[i];
        return RG_OK;
    };
    for (const auto &g : groups) {
        const size_t first = g.first, cnt = g.second;  // (a group holds at least one file)
        AlbumFold fold;
        fold.d_packs = carry + RG_ALBUMS_PACK_STRIDE;
        fold.pack_of.resize(cnt);
        for (size_t i = 0; i < cnt; ++i) {
            const size_t a = album_of[first + i];
            if (fold.album_of_pack.empty() || fold.album_of_pack.back() != a) fold.album_of_pack.push_back(a);
            fold.pack_of[i] = (int32_t)(fold.album_of_pack.size() - 1);
        }
        fold.n_packs = fold.album_of_pack.size();
        const size_t a_first = fold.album_of_pack.front(), a_last = fold.album_of_pack.back();
        fold.carried = album_first[a_first] < first;
        int rc = fold_init(c, &fold);
        if (rc != RG_OK) return rc;
        rc = analyze_tracks_group(c, paths, first, cnt, track_index, tracks_out, status_out, &fold);
        if (rc != RG_OK) return rc;
        const bool continues = album_first[a_last + 1] > first + cnt;
        const size_t n_fin = fold.n_packs - (continues ? 1 : 0);
        RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
        if (n_fin) {
            RG_HIP(c, rg_launch_album_results(fold.d_packs, 0, (uint32_t)n_fin, c->d_albums_res.p, s));
            RG_HIP(c, hipMemcpyAsync(c->h_albums_res.p, c->d_albums_res.p, n_fin * sizeof(rg_album_result), hipMemcpyDeviceToHost, s));
        }
        if (continues)
            RG_HIP(c, hipMemcpyAsync(carry, fold.d_packs + (fold.n_packs - 1) * (size_t)RG_ALBUMS_PACK_STRIDE,
                                     (size_t)RG_ALBUMS_PACK_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        *files_done = first + cnt;
        for (size_t k = 0; k < n_fin; ++k) {
            const size_t a = fold.album_of_pack[k];
            album_status_out[a] = album_status(a);
            if (album_status_out[a] == RG_OK) albums_out[a] = c->h_albums_res.p[k];
            done[a] = 1;
        }
    }
    // albums without files (they have no pack): what rg_analyze_album gives for n = 0, the read-out of an empty pack
    if (std::find(done.begin(), done.end(), 0) != done.end()) {
        RG_HIP(c, hipMemsetAsync(carry, 0, (size_t)RG_ALBUMS_PACK_STRIDE * sizeof(uint32_t), s));
        RG_HIP(c, rg_launch_album_results(carry, 0, 1, c->d_albums_res.p, s));
        RG_HIP(c, hipMemcpyAsync(c->h_albums_res.p, c->d_albums_res.p, sizeof(rg_album_result), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t a = 0; a < n_albums; ++a)
            if (!done[a]) {
                albums_out[a] = c->h_albums_res.p[0];
                album_status_out[a] = RG_OK;
                done[a] = 1;
            }
    }
    return RG_OK;
}

extern "C" int rg_analyze_albums(rg_ctx *c, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                                 int32_t track_index, rg_track_result *tracks_out, int32_t *status_out, rg_album_result *albums_out,
                                 int32_t *album_status_out) {
    if (!c) return RG_ERR_INVALID_ARG;
    if ((n && (!paths || !tracks_out || !status_out)) || (n_albums && (!albums_out || !album_status_out)))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_analyze_albums: null input or output array");
    std::string why;
    if (rg_albums_check(album_first, n_albums, n, &why) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_analyze_albums: %s", why.c_str());
    c->file_errors.assign(n, std::string());
    for (size_t a = 0; a < n_albums; ++a) memset(&albums_out[a], 0, sizeof albums_out[a]);
    std::vector<char> done(n_albums, 0);
    size_t files_done = 0;
    int rc = rg_bind_device(c);
    if (rc == RG_OK)
        rc = analyze_albums_impl(c, paths, n, album_first, n_albums, track_index, tracks_out, status_out, albums_out, album_status_out,
                                 done, &files_done);
    if (rc != RG_OK) {  // the call itself failed (a device error): what it did not finish carries the call's code and text
        const std::string text = c->err;
        for (size_t i = files_done; i < n; ++i) {
            memset(&tracks_out[i], 0, sizeof tracks_out[i]);
            status_out[i] = rc;
            c->file_errors[i] = text;
        }
        for (size_t a = 0; a < n_albums; ++a)
            if (!done[a]) {
                memset(&albums_out[a], 0, sizeof albums_out[a]);
                album_status_out[a] = rc;
            }
        c->err = text;
    }
    return rc;
}

// ---- rg_flac_verify (include/mp3rgain_amd_flac.h) ---------------------------------------------------------------------------
// one group of the call: files [first, first + n).  The route is the analysis's: load_many, stage_loaded, then the hash of
// what lies in the arena (device decoder) or of the host decoder's PCM (tuning key 14 = 0), then the per-file records.
static int flac_verify_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, rg_flac_verify_result *out) {
    paths += first;
    out += first;
    std::vector<LoadedAudio> &in = file_pool(c, n);
    std::vector<int> rcs;
    std::vector<std::string> errs;
    // no decoder command here: what this library does not decode itself is not a FLAC stream it could verify
    std::string cmd;
    cmd.swap(c->decoder_cmd);
    int rc = load_many(c, paths, n, &in, &rcs, &errs, nullptr);
    cmd.swap(c->decoder_cmd);
    if (rc != RG_OK) return rc;
    // everything that loaded and is not a WAV stream goes through the staging, as in an analysis call (what the loader
    // pipeline has put into the arena already stays accounted for); only the FLAC streams are hashed
    std::vector<size_t> slot;
    for (size_t i = 0; i < n; ++i) {
        out[i].status = rcs[i];
        c->file_errors[first + i] = errs[i];
        if (rcs[i] != RG_OK) continue;
        if (in[i].kind == LoadedAudio::Wav) {
            out[i].status = RG_ERR_FORMAT;
            c->file_errors[first + i] = std::string("Not a native FLAC stream: ") + paths[i];
            continue;
        }
        slot.push_back(i);
    }
    if (slot.empty()) return RG_OK;
    for (size_t k = 0; k < slot.size(); ++k)
        if (slot[k] != k) std::swap(in[k], in[slot[k]]);
    auto fail_all = [&](int code) {
        for (size_t k = 0; k < slot.size(); ++k) {
            memset(&out[slot[k]], 0, sizeof out[slot[k]]);
            out[slot[k]].status = code;
            c->file_errors[first + slot[k]] = c->err;
        }
        return RG_OK;
    };
    std::vector<rg_track_desc> descs;
    std::vector<FlacCounts> counts;
    size_t arena_bytes = 0;
    rc = stage_loaded(c, in, slot.size(), &descs, &arena_bytes, &counts);
    if (rc != RG_OK) return fail_all(rc);
    std::vector<RgFlacMd5Rec> recs;
    std::vector<size_t> rec_of;  // record -> position in the batch
    for (size_t k = 0; k < slot.size(); ++k) {
        rg_flac_verify_result &r = out[slot[k]];
        if (in[k].kind != LoadedAudio::Flac) {
            r.status = RG_ERR_FORMAT;
            c->file_errors[first + slot[k]] = std::string("Not a native FLAC stream: ") + paths[slot[k]];
            continue;
        }
        rg_flac_info si;
        (void)rg_flac_scan(in[k].file_bytes.data(), in[k].file_bytes.size(), &si);  // (load_flac has walked this stream)
        if (rg_flac_stream_md5(in[k].file_bytes.data(), in[k].file_bytes.size(), r.md5_stream) == 1) r.flags |= RG_FLAC_VERIFY_HAS_SIGNATURE;
        r.frames = descs[k].frames;
        r.total_samples = si.total_samples;
        r.audio_frames = counts[k].decoded;
        r.dropped_frames = counts[k].dropped;
        RgFlacMd5Rec rec;
        if (in[k].flac_frames.empty()) {  // the host decoder's PCM, in the arena's format (or a stream without frames)
            rg_track_desc d = descs[k];
            d.offset_bytes = 0;
            rc = rg_flac_md5_record(c, slot[k], d, in[k].flac_bps, in[k].flac_pcm.data(), in[k].flac_pcm.size(), &rec);
            if (rc != RG_OK) return fail_all(rc);
            rg_flac_md5_host(rec, r.md5_decoded);
            continue;
        }
        rc = rg_flac_md5_record(c, slot[k], descs[k], in[k].flac_bps, c->d_arena.p, arena_bytes, &rec);
        if (rc != RG_OK) return fail_all(rc);
        recs.push_back(rec);
        rec_of.push_back(k);
    }
    if (!recs.empty()) {  // on the stream the decode ran on
        std::vector<uint8_t> dig(recs.size() * 16);
        rc = rg_flac_md5_device(c, recs.data(), recs.size(), dig.data(), c->user_attached ? c->user_stream : c->slot().stream);
        if (rc != RG_OK) return fail_all(rc);
        for (size_t j = 0; j < recs.size(); ++j) memcpy(out[slot[rec_of[j]]].md5_decoded, &dig[16 * j], 16);
    }
    for (size_t k = 0; k < slot.size(); ++k) {
        rg_flac_verify_result &r = out[slot[k]];
        if (r.status != RG_OK) continue;
        if ((r.flags & RG_FLAC_VERIFY_HAS_SIGNATURE) && memcmp(r.md5_stream, r.md5_decoded, 16) == 0) r.flags |= RG_FLAC_VERIFY_MD5_MATCH;
        if (r.total_samples == 0 || r.total_samples == r.frames) r.flags |= RG_FLAC_VERIFY_LENGTH_MATCH;
        if (r.dropped_frames == 0) r.flags |= RG_FLAC_VERIFY_COMPLETE;
    }
    return RG_OK;
}

extern "C" int rg_flac_verify(rg_ctx *c, const char *const *paths, size_t n, rg_flac_verify_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    c->file_errors.assign(n, std::string());
    if (n) memset(out, 0, n * sizeof *out);
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    try {
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        for (const auto &g : groups) {
            rc = flac_verify_group(c, paths, g.first, g.second, out);
            if (rc != RG_OK) return rc;
        }
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
    return RG_OK;
}

// ---- rg_mp3_verify (include/mp3rgain_amd_mp3verify.h) ---------------------------------------------------------------------
// one group of the call.  The decode side is the analysis's (load_many without a decoder command, stage_loaded), so how many
// frames were dropped is the route's own verdict; the loader keeps the bytes of MPEG streams as read while this runs.  The
// checksums: one upload of the group's bytes with their range and frame tables and the kernels of rg_mp3_crc.hip, on the
// stream the decode ran on; with tuning key 6 = 0 (the host decoder) the host twin.
static int mp3_verify_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, rg_mp3_verify_result *out) {
    paths += first;
    out += first;
    std::vector<LoadedAudio> &in = file_pool(c, n);
    std::vector<int> rcs;
    std::vector<std::string> errs;
    struct Quiet {  // no decoder command; MPEG bytes kept
        rg_ctx *c;
        std::string cmd;
        explicit Quiet(rg_ctx *c) : c(c) { cmd.swap(c->decoder_cmd); c->keep_mpeg_bytes = true; }
        ~Quiet() { cmd.swap(c->decoder_cmd); c->keep_mpeg_bytes = false; }
    };
    int rc;
    {
        Quiet q(c);
        rc = load_many(c, paths, n, &in, &rcs, &errs, nullptr);
    }
    if (rc != RG_OK) return rc;
    std::vector<size_t> slot;
    for (size_t i = 0; i < n; ++i) {
        out[i].status = rcs[i];
        c->file_errors[first + i] = errs[i];
        if (rcs[i] != RG_OK) continue;
        const bool mpeg = in[i].kind == LoadedAudio::Planar || in[i].kind == LoadedAudio::Split || in[i].kind == LoadedAudio::Staged;
        if (!mpeg || in[i].mpeg_in_mp4) {
            out[i].status = RG_ERR_FORMAT;
            c->file_errors[first + i] = std::string("Not a bare MPEG Layer III stream: ") + paths[i];
            continue;
        }
        slot.push_back(i);
    }
    if (slot.empty()) return RG_OK;
    for (size_t k = 0; k < slot.size(); ++k)
        if (slot[k] != k) std::swap(in[k], in[slot[k]]);
    const size_t m = slot.size();
    auto fail_all = [&](int code) {
        for (size_t k = 0; k < m; ++k) {
            memset(&out[slot[k]], 0, sizeof out[slot[k]]);
            out[slot[k]].status = code;
            c->file_errors[first + slot[k]] = c->err;
        }
        return RG_OK;
    };
    std::vector<rg_track_desc> descs;
    size_t arena_bytes = 0;
    rc = stage_loaded(c, in, m, &descs, &arena_bytes);
    if (rc != RG_OK) return fail_all(rc);
    std::vector<RgMp3VerifyPlan> plans(m);
    std::vector<uint32_t> dropped(m, 0);
    std::vector<char> live(m, 0);
    for (size_t k = 0; k < m; ++k) {
        const LoadedAudio &la = in[k];
        if (rg_mp3_verify_plan(la.file_bytes.data(), la.file_bytes.size(), &plans[k]) != RG_OK) {
            out[slot[k]].status = RG_ERR_FORMAT;
            c->file_errors[first + slot[k]] = std::string("Not a bare MPEG Layer III stream: ") + paths[slot[k]];
            continue;
        }
        live[k] = 1;
        const uint32_t spf = plans[k].si.samples_per_frame ? plans[k].si.samples_per_frame : 1152;
        dropped[k] = la.kind == LoadedAudio::Staged ? (uint32_t)((la.walked_frames - std::min(la.walked_frames, la.frames)) / spf) : la.mp3_skipped;
    }
    std::vector<uint16_t> music(m, 0);
    std::vector<uint32_t> failed(m, 0);
    if (c->gpu_mp3_decode == 0) {  // the host twin
        for (size_t k = 0; k < m; ++k) {
            if (!live[k]) continue;
            const uint8_t *d = in[k].file_bytes.data();
            music[k] = rg_mp3_crc_range_host(d, plans[k].music_off, plans[k].music_len);
            for (uint64_t o : plans[k].prot) failed[k] += rg_mp3_frame_crc_host(d, in[k].file_bytes.size(), o) ? 0u : 1u;
        }
    } else {
        std::vector<const uint8_t *> parts(m);
        std::vector<uint64_t> part_off(m), part_len(m), r_off(m), r_len(m), f_off;
        std::vector<size_t> f_of;
        uint64_t total = 0;
        for (size_t k = 0; k < m; ++k) {
            parts[k] = in[k].file_bytes.data();
            part_off[k] = total;
            part_len[k] = live[k] ? in[k].file_bytes.size() : 0;
            r_off[k] = total + (live[k] ? plans[k].music_off : 0);
            r_len[k] = live[k] ? plans[k].music_len : 0;
            if (live[k])
                for (uint64_t o : plans[k].prot) {
                    f_off.push_back(total + o);
                    f_of.push_back(k);
                }
            total = (total + part_len[k] + 15) & ~(uint64_t)15;
        }
        std::vector<uint8_t> ok(f_off.size() ? f_off.size() : 1);
        RgMp3CrcJob job;
        job.parts = parts.data();
        job.part_off = part_off.data();
        job.part_len = part_len.data();
        job.n_parts = m;
        job.nbytes = total;
        job.range_off = r_off.data();
        job.range_len = r_len.data();
        job.n_ranges = m;
        job.frame_off = f_off.data();
        job.n_frames = f_off.size();
        job.crc_out = music.data();
        job.ok_out = ok.data();
        rc = rg_mp3_crc_device(c, job, c->user_attached ? c->user_stream : c->slot().stream);
        if (rc != RG_OK) return fail_all(rc);
        for (size_t j = 0; j < f_off.size(); ++j) failed[f_of[j]] += ok[j] ? 0u : 1u;
    }
    for (size_t k = 0; k < m; ++k)
        if (live[k]) rg_mp3_verify_fill(in[k].file_bytes.data(), in[k].file_bytes.size(), plans[k], dropped[k], music[k], failed[k], &out[slot[k]]);
    return RG_OK;
}

extern "C" int rg_mp3_verify(rg_ctx *c, const char *const *paths, size_t n, rg_mp3_verify_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    c->file_errors.assign(n, std::string());
    if (n) memset(out, 0, n * sizeof *out);
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    try {
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        for (const auto &g : groups) {
            rc = mp3_verify_group(c, paths, g.first, g.second, out);
            if (rc != RG_OK) return rc;
        }
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
    return RG_OK;
}

// find_peak_amplitude (src/replaygain.rs:1140-1249): max |x| over ALL channels, no loudness analysis
// ---- rg_rip_checksums (include/mp3rgain_amd_rip.h) --------------------------------------------------------------------------
// one group of the call: files [first, first + n).  The route is rg_flac_verify's -- load_many without a decoder command,
// stage_loaded -- except that 16-bit stereo WAV streams are kept.  Whatever route put a track's PCM into the arena (device
// FLAC decoder, the host decoder's planes by copy, the WAV de-interleave), the two kernels of rg_rip_crc.hip read it there, on
// the stream the decode ran on, so tuning key 14 cannot show in the records.
static int rip_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const uint32_t *track_flags, rg_rip_result *out) {
    paths += first;
    out += first;
    if (track_flags) track_flags += first;
    std::vector<LoadedAudio> &in = file_pool(c, n);
    std::vector<int> rcs;
    std::vector<std::string> errs;
    std::string cmd;
    cmd.swap(c->decoder_cmd);
    int rc = load_many(c, paths, n, &in, &rcs, &errs, nullptr);
    cmd.swap(c->decoder_cmd);
    if (rc != RG_OK) return rc;
    auto refuse = [&](size_t i, const std::string &why) {
        out[i].status = RG_ERR_FORMAT;
        c->file_errors[first + i] = "No rip checksums (" + why + "): " + paths[i];
    };
    // everything that loaded goes through the staging, as in an analysis call (what the loader pipeline has put into the arena
    // already stays accounted for), except WAV streams that take no part: the staging cannot lay out every kind of them
    std::vector<size_t> slot;
    for (size_t i = 0; i < n; ++i) {
        out[i].status = rcs[i];
        c->file_errors[first + i] = errs[i];
        if (rcs[i] != RG_OK) continue;
        if (in[i].kind == LoadedAudio::Wav) {
            rg_wav_info w;
            if (rg_wav_parse(in[i].wav.data(), in[i].wav.size(), &w) != RG_OK) {
                out[i].status = RG_ERR_FORMAT;
                c->file_errors[first + i] = std::string("Failed to probe format: ") + paths[i];
                continue;
            }
            if (w.sample_format != 1 || w.bits_per_sample != 16 || w.channels != 2) {
                refuse(i, std::to_string(w.channels) + " channel(s) of " + std::to_string(w.bits_per_sample) + "-bit " +
                              (w.sample_format == 3 ? "float" : "integer") + " PCM, not 2 of 16-bit integer");
                continue;
            }
        }
        slot.push_back(i);
    }
    if (slot.empty()) return RG_OK;
    for (size_t k = 0; k < slot.size(); ++k)
        if (slot[k] != k) std::swap(in[k], in[slot[k]]);
    auto fail_all = [&](int code) {
        for (size_t k = 0; k < slot.size(); ++k) {
            memset(&out[slot[k]], 0, sizeof out[slot[k]]);
            out[slot[k]].status = code;
            c->file_errors[first + slot[k]] = c->err;
        }
        return RG_OK;
    };
    std::vector<rg_track_desc> descs;
    std::vector<FlacCounts> counts;
    size_t arena_bytes = 0;
    rc = stage_loaded(c, in, slot.size(), &descs, &arena_bytes, &counts);
    if (rc != RG_OK) return fail_all(rc);
    std::vector<RgRipTrack> recs;
    std::vector<size_t> rec_of;  // record -> position in the batch
    for (size_t k = 0; k < slot.size(); ++k) {
        const size_t i = slot[k];
        if (in[k].kind != LoadedAudio::Wav && in[k].kind != LoadedAudio::Flac) {
            refuse(i, "an MPEG stream, not a WAV or native FLAC stream");
            continue;
        }
        if (in[k].kind == LoadedAudio::Flac && (in[k].flac_bps != 16 || in[k].channels != 2)) {
            refuse(i, std::to_string(in[k].channels) + " channel(s) of " + std::to_string(in[k].flac_bps) + " bits per sample, not 2 of 16");
            continue;
        }
        RgRipTrack rec;
        char err[256] = "";
        rc = rg_rip_track_record(i, descs[k], track_flags ? track_flags[i] : 0u, arena_bytes, &rec, err, sizeof err);
        if (rc == RG_ERR_FORMAT) {
            refuse(i, err);
            continue;
        }
        if (rc != RG_OK) return fail_all(rg_set_err(c, rc, "%s", err));
        recs.push_back(rec);
        rec_of.push_back(k);
    }
    if (recs.empty()) return RG_OK;
    std::vector<RgRipSums> sums(recs.size());
    rc = rg_rip_device(c, c->d_arena.p, recs.data(), recs.size(), sums.data(), c->user_attached ? c->user_stream : c->slot().stream);
    if (rc != RG_OK) return fail_all(rc);
    for (size_t j = 0; j < recs.size(); ++j) {
        const size_t k = rec_of[j];
        rg_rip_fill(sums[j], descs[k].frames, descs[k].sample_rate, counts[k].dropped, &out[slot[k]]);
    }
    return RG_OK;
}

extern "C" int rg_rip_checksums(rg_ctx *c, const char *const *paths, size_t n, const uint32_t *track_flags, rg_rip_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    c->file_errors.assign(n, std::string());
    if (n) memset(out, 0, n * sizeof *out);
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    try {
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        for (const auto &g : groups) {
            rc = rip_group(c, paths, g.first, g.second, track_flags, out);
            if (rc != RG_OK) return rc;
        }
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
    return RG_OK;
}

extern "C" int rg_find_peak_amplitude(rg_ctx *c, const char *path, rg_peak_result *out) {
    if (!c || !out) return RG_ERR_INVALID_ARG;
    rg_track_desc desc;
    size_t arena_bytes = 0;
    const int rc = load_and_stage_one(c, path, -1, &desc, &arena_bytes);
    if (rc != RG_OK) return rc;
    // the arena was produced on the stream rg_find_peak_pcm uses, so no further ordering is needed
    return rg_find_peak_pcm(c, &desc, c->d_arena.p, arena_bytes, 1, out);
}

// ---- EBU R 128 (include/mp3rgain_amd_r128.h): the same loaders, decoders and groups; the analysis is rg_r128.hip's ---------
// one group of files -> their results; album: the first failing file in input order aborts (its index in *failed), else a
// failing file fails alone
// (kept_tr / kept_slot / kept_e, rg_r128_analyze_albums: the device descriptors of the files that were analysed, their indices in
// the group, and their hop energies in a buffer that is the caller's to free)
static int r128_files_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, int32_t track_index, int want_tp, bool album,
                            rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out /* tracks only; may be nullptr */,
                            std::vector<RgR128TrackDev> *kept_tr = nullptr, std::vector<size_t> *kept_slot = nullptr,
                            double **kept_e = nullptr) {
    paths += first;
    out += first;
    if (dyn_out) {
        dyn_out += first;
        memset(dyn_out, 0, n * sizeof *dyn_out);
    }
    std::vector<LoadedAudio> &in = file_pool(c, n);
    std::vector<int> rcs;
    std::vector<std::string> errs;
    c->file_track_index = track_index;
    int rc = load_many(c, paths, n, &in, &rcs, &errs, nullptr);
    c->file_track_index = -1;
    if (rc != RG_OK) return rc;
    const bool layout = rg_r128_channel_mode(c) == RG_R128_CHANNELS_LAYOUT;
    std::vector<size_t> slot;
    for (size_t i = 0; i < n; ++i) {
        memset(&out[i], 0, sizeof out[i]);
        std::string msg;
        int frc = file_outcome(in[i], rcs[i], errs[i], paths[i], track_index, &msg, true);
        if (frc == RG_OK && !stageable(in[i])) {
            frc = RG_ERR_FORMAT;
            msg = std::string("Failed to probe format: ") + paths[i];
        }
        if (frc == RG_OK && layout) {  // a layout has 1 to 8 channels
            uint32_t channels = in[i].channels;
            if (in[i].kind == LoadedAudio::Wav) {
                rg_wav_info wi;
                channels = rg_wav_parse(in[i].wav.data(), in[i].wav.size(), &wi) == RG_OK ? wi.channels : 0;
            }
            if (channels < 1 || channels > 8) {
                char m[128];
                snprintf(m, sizeof m, "Unsupported channel count for layout analysis: %u (1 to 8)", channels);
                frc = RG_ERR_INVALID_ARG;
                msg = m;
            }
        }
        if (frc != RG_OK && album) return rg_set_err(c, frc, "%s", msg.c_str());
        if (status_out) {
            status_out[first + i] = frc;
            c->file_errors[first + i] = msg;
        }
        if (frc == RG_OK) slot.push_back(i);
    }
    if (slot.empty()) return RG_OK;
    std::vector<rg_r128_dynamics> dyn(dyn_out ? slot.size() : 0);
    if (kept_tr) kept_tr->resize(slot.size());
    rc = run_good_files(c, in, slot, out, [&](const rg_track_desc *descs, size_t k, size_t arena_bytes, rg_r128_track_result *res) {
        // LAYOUT mode: every file's weights from its container's channel mask (file j of the batch is in[j] by now)
        std::vector<rg_r128_channel_weights> weights(layout ? k : 0);
        for (size_t j = 0; j < weights.size(); ++j) {
            const uint32_t mask = in[j].kind == LoadedAudio::Wav ? wav_channel_mask(in[j].wav.data(), in[j].wav.size()) : 0u;
            if (rg_r128_layout_weights(descs[j].channels, mask, &weights[j]) != RG_OK)
                return rg_set_err(c, RG_ERR_INVALID_ARG, "Unsupported channel count for layout analysis: %u (1 to 8)", descs[j].channels);
        }
        return rg_r128_run(c, descs, k, c->d_arena.p, arena_bytes, want_tp, album ? 1 : 0, res, nullptr, dyn_out ? dyn.data() : nullptr, nullptr,
                           kept_tr ? kept_tr->data() : nullptr, kept_e, layout ? weights.data() : nullptr);
    });
    if (rc != RG_OK) {
        if (album) return rc;
        if (kept_tr) kept_tr->clear();
        fail_batch(c, slot, first, rc, status_out + first);
        return RG_OK;
    }
    if (kept_slot) *kept_slot = slot;
    for (size_t k = 0; k < slot.size() && dyn_out; ++k) dyn_out[slot[k]] = dyn[k];
    return RG_OK;
}

static int r128_tracks(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                       rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out) {
    if (!c || (n && (!paths || !out || !status_out))) return RG_ERR_INVALID_ARG;
    c->file_errors.assign(n, std::string());
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    for (const auto &g : groups) {
        rc = r128_files_group(c, paths, g.first, g.second, track_index, want_true_peak, false, out, status_out, dyn_out);
        if (rc != RG_OK) return rc;
    }
    return RG_OK;
}

static int r128_album(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                      rg_r128_track_result *tracks_out, rg_r128_album_result *album_out, rg_r128_dynamics *dyn_out,
                      rg_r128_dynamics *album_dyn_out) {
    if (!c || (n && (!paths || !tracks_out)) || !album_out) return RG_ERR_INVALID_ARG;
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    rg_r128_album_reset(c);
    for (const auto &g : groups) {
        rc = r128_files_group(c, paths, g.first, g.second, track_index, want_true_peak, true, tracks_out, nullptr, nullptr);
        if (rc != RG_OK) {
            rg_r128_album_reset(c);
            return rc;
        }
    }
    return rg_r128_album_end(c, want_true_peak, album_out, dyn_out, album_dyn_out, nullptr);
}

extern "C" int rg_r128_analyze_tracks(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                      rg_r128_track_result *out, int32_t *status_out) {
    return r128_tracks(c, paths, n, track_index, want_true_peak, out, status_out, nullptr);
}

extern "C" int rg_r128_analyze_album(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                     rg_r128_track_result *tracks_out, rg_r128_album_result *album_out) {
    return r128_album(c, paths, n, track_index, want_true_peak, tracks_out, album_out, nullptr, nullptr);
}

extern "C" int rg_r128_analyze_tracks_dynamics(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                               rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out) {
    if (c && n && !dyn_out) return rg_set_err(c, RG_ERR_INVALID_ARG, "null dyn_out");
    return r128_tracks(c, paths, n, track_index, want_true_peak, out, status_out, dyn_out);
}

extern "C" int rg_r128_analyze_album_dynamics(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                              rg_r128_track_result *tracks_out, rg_r128_album_result *album_out,
                                              rg_r128_dynamics *dyn_out, rg_r128_dynamics *album_dyn_out) {
    if (c && ((n && !dyn_out) || !album_dyn_out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "null dynamics output");
    return r128_album(c, paths, n, track_index, want_true_peak, tracks_out, album_out, dyn_out, album_dyn_out);
}

// Many albums in one call: rg_r128_analyze_tracks' groups over the whole list, every group's hop energies kept on the device.
// After each group the albums whose last file lies in the groups taken so far are gated in one album stage
// (rg_r128_albums.hip); a group's energies are freed as soon as no unfinished album has tracks in them, so what is live is
// the current group plus the groups the one straddling album spans.  Per album the first failing file in input order decides;
// the good files of such an album keep their results (and, with dynamics, get theirs from the same stage).
static int r128_albums_impl(rg_ctx *c, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                            int32_t track_index, int want_tp, rg_r128_track_result *tracks_out, int32_t *status_out,
                            rg_r128_album_result *albums_out, int32_t *album_status_out, bool dynamics, rg_r128_dynamics *dyn_out,
                            rg_r128_dynamics *albums_dyn_out, std::vector<char> &done, size_t *files_done,
                            std::vector<std::pair<size_t, double *>> &bufs /* (end of the group, its energies) */) {
    std::vector<std::pair<size_t, size_t>> groups;
    file_groups(c, paths, n, &groups);
    std::vector<RgR128TrackDev> kept(n);  // by file; valid where the file's status is RG_OK
    size_t next_album = 0;                // the albums before it are finished
    // albums [next_album, a_end): one stage over their files (the failed albums' good files after the last album's)
    auto finish = [&](size_t a_end) -> int {
        std::vector<RgR128TrackDev> tr;
        std::vector<rg_r128_track_result> res;
        std::vector<size_t> seg(1, 0), seg_album, file_of;
        auto take = [&](size_t i) {
            tr.push_back(kept[i]);
            res.push_back(tracks_out[i]);
            file_of.push_back(i);
        };
        for (size_t a = next_album; a < a_end; ++a) {
            album_status_out[a] = RG_OK;
            for (size_t i = album_first[a]; i < album_first[a + 1] && album_status_out[a] == RG_OK; ++i) album_status_out[a] = status_out[i];
            if (album_status_out[a] != RG_OK) continue;
            for (size_t i = album_first[a]; i < album_first[a + 1]; ++i) take(i);
            seg.push_back(tr.size());
            seg_album.push_back(a);
        }
        if (dynamics)
            for (size_t a = next_album; a < a_end; ++a)
                for (size_t i = album_first[a]; i < album_first[a + 1] && album_status_out[a] != RG_OK; ++i)
                    if (status_out[i] == RG_OK) take(i);
        const size_t k = seg_album.size();
        std::vector<rg_r128_album_result> alb(k + 1);
        std::vector<rg_r128_dynamics> dyn(tr.size() + 1), adyn(k + 1);
        const int rc = rg_r128_albums_stage(c, tr.data(), res.data(), tr.size(), seg.data(), k, want_tp, alb.data(),
                                            dynamics ? dyn.data() : nullptr, dynamics ? adyn.data() : nullptr, nullptr);
        if (rc != RG_OK) return rc;
        for (size_t q = 0; q < k; ++q) {
            albums_out[seg_album[q]] = alb[q];
            if (dynamics) albums_dyn_out[seg_album[q]] = adyn[q];
        }
        for (size_t j = 0; j < tr.size() && dynamics; ++j) dyn_out[file_of[j]] = dyn[j];
        for (size_t a = next_album; a < a_end; ++a) done[a] = 1;
        next_album = a_end;
        return RG_OK;
    };
    for (const auto &g : groups) {
        const size_t first = g.first, end = g.first + g.second;
        std::vector<RgR128TrackDev> tr;
        std::vector<size_t> slot;
        double *e = nullptr;
        int rc = r128_files_group(c, paths, first, g.second, track_index, want_tp, false, tracks_out, status_out, nullptr, &tr, &slot, &e);
        if (e) bufs.push_back(std::make_pair(end, e));
        if (rc != RG_OK) return rc;
        for (size_t k = 0; k < tr.size(); ++k) kept[first + slot[k]] = tr[k];
        size_t a_end = next_album;
        while (a_end < n_albums && album_first[a_end + 1] <= end) ++a_end;
        if (a_end > next_album) {
            rc = finish(a_end);
            if (rc != RG_OK) return rc;
        }
        *files_done = end;
        const size_t live_from = next_album < n_albums ? album_first[next_album] : n;  // the first file of an unfinished album
        while (!bufs.empty() && bufs.front().first <= live_from) {
            (void)hipFree(bufs.front().second);
            bufs.erase(bufs.begin());
        }
    }
    if (next_album < n_albums) return finish(n_albums);  // (albums without files after the last group, or a call without files)
    return RG_OK;
}

static int r128_albums(rg_ctx *c, const char *fn, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                       int32_t track_index, int want_tp, rg_r128_track_result *tracks_out, int32_t *status_out,
                       rg_r128_album_result *albums_out, int32_t *album_status_out, bool dynamics, rg_r128_dynamics *dyn_out,
                       rg_r128_dynamics *albums_dyn_out) {
    if (!c) return RG_ERR_INVALID_ARG;
    if ((n && (!paths || !tracks_out || !status_out || (dynamics && !dyn_out))) ||
        (n_albums && (!albums_out || !album_status_out || (dynamics && !albums_dyn_out))))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: null input or output array", fn);
    std::string why;
    if (rg_albums_check(album_first, n_albums, n, &why) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: %s", fn, why.c_str());
    c->file_errors.assign(n, std::string());
    for (size_t a = 0; a < n_albums; ++a) {
        memset(&albums_out[a], 0, sizeof albums_out[a]);
        if (dynamics) memset(&albums_dyn_out[a], 0, sizeof albums_dyn_out[a]);
    }
    if (dynamics && n) memset(dyn_out, 0, n * sizeof *dyn_out);
    std::vector<char> done(n_albums, 0);
    size_t files_done = 0;
    std::vector<std::pair<size_t, double *>> bufs;
    int rc = rg_bind_device(c);
    if (rc == RG_OK)
        rc = r128_albums_impl(c, paths, n, album_first, n_albums, track_index, want_tp, tracks_out, status_out, albums_out,
                              album_status_out, dynamics, dyn_out, albums_dyn_out, done, &files_done, bufs);
    for (const auto &b : bufs) (void)hipFree(b.second);
    if (rc != RG_OK) {  // the call itself failed (a device error): what it did not finish carries the call's code and text
        const std::string text = c->err;
        for (size_t i = files_done; i < n; ++i) {
            memset(&tracks_out[i], 0, sizeof tracks_out[i]);
            if (dynamics) memset(&dyn_out[i], 0, sizeof dyn_out[i]);
            status_out[i] = rc;
            c->file_errors[i] = text;
        }
        for (size_t a = 0; a < n_albums; ++a)
            if (!done[a]) {
                memset(&albums_out[a], 0, sizeof albums_out[a]);
                if (dynamics) memset(&albums_dyn_out[a], 0, sizeof albums_dyn_out[a]);
                album_status_out[a] = rc;
            }
        c->err = text;
    }
    return rc;
}

extern "C" int rg_r128_analyze_albums(rg_ctx *c, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                                      int32_t track_index, int want_true_peak, rg_r128_track_result *tracks_out, int32_t *status_out,
                                      rg_r128_album_result *albums_out, int32_t *album_status_out) {
    return r128_albums(c, "rg_r128_analyze_albums", paths, n, album_first, n_albums, track_index, want_true_peak, tracks_out, status_out,
                       albums_out, album_status_out, false, nullptr, nullptr);
}

extern "C" int rg_r128_analyze_albums_dynamics(rg_ctx *c, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                                               int32_t track_index, int want_true_peak, rg_r128_track_result *tracks_out,
                                               int32_t *status_out, rg_r128_album_result *albums_out, int32_t *album_status_out,
                                               rg_r128_dynamics *dyn_out, rg_r128_dynamics *albums_dyn_out) {
    return r128_albums(c, "rg_r128_analyze_albums_dynamics", paths, n, album_first, n_albums, track_index, want_true_peak, tracks_out,
                       status_out, albums_out, album_status_out, true, dyn_out, albums_dyn_out);
}
