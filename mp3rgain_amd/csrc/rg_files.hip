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
// This file holds the ReplayGain and EBU R 128 entry points and their group helpers; the rest of the file layer: rg_wav.hip,
// rg_file_load.hip, rg_file_stage.hip, rg_mp3_pipe.hip, rg_file_verify.hip (the verify and rip entry points), rg_file_hooks.hip
// (shared declarations, the call driver and the group route: rg_files.h).
#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>

#include "rg_albums.h"
#include "rg_files.h"
#include "rg_r128.h"

using namespace rgf;

// One file, loaded and laid into the arena: *desc describes it, *file_type (if given) is what detect_file_type makes of it.
// Some(idx) selects among the audio tracks of a container (src/replaygain.rs:838-851); a WAV stream has one
static int load_and_stage_one(rg_ctx *c, const char *path, int32_t track_index, rg_track_desc *desc, size_t *arena_bytes,
                              uint32_t *file_type = nullptr) {
    std::vector<LoadedAudio> &pool = file_pool(c, 1);
    int rc = load_one(c, path, &pool, LoadOpts{track_index});
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

// Album parts of a group of n files, after loading: if every file was analysed as a part of its chunk (`parts`: the group's, or
// null if it had none) the results are on their way to the host and, in album mode, the packs are on the device.  *stand: the
// parts' results are the files' (out[i] <- file i, file_type included); else a file did not come through the pipeline, or a
// track is flagged and the plain route has to repeat it on the order-faithful kernel: nothing was taken.
static int take_parts(rg_ctx *c, const PartsRun *parts, const std::vector<LoadedAudio> &in, size_t n, rg_track_result *out, bool *stand) {
    *stand = false;
    if (!parts || parts->broken || parts->file_of.size() != n) return RG_OK;
    RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
    const rg_track_result *res = c->h_part_results.p;
    for (size_t j = 0; j < n; ++j)
        if (c->kernel_variant == 0 && (res[j].flags & RG_TRACK_FLAG_IMPRECISE)) return RG_OK;
    for (size_t j = 0; j < n; ++j) {
        const size_t i = parts->file_of[j];
        out[i] = res[j];
        out[i].file_type = in[i].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
    }
    *stand = true;
    return RG_OK;
}

// The tail of a many-albums call that failed as a whole (a device error, no memory): what it did not finish -- the files from
// files_done on, the albums not `done` -- is zeroed and carries the call's code and text, which c->err keeps.
// (dyn_out / albums_dyn_out: the R 128 calls with dynamics, else null)
template <typename Track, typename Album>
static int fail_rest(rg_ctx *c, int rc, size_t files_done, size_t n, const std::vector<char> &done, Track *tracks_out, int32_t *status_out,
                     Album *albums_out, int32_t *album_status_out, rg_r128_dynamics *dyn_out = nullptr, rg_r128_dynamics *albums_dyn_out = nullptr) {
    const std::string text = c->err;
    for (size_t i = files_done; i < n; ++i) {
        memset(&tracks_out[i], 0, sizeof tracks_out[i]);
        if (dyn_out) memset(&dyn_out[i], 0, sizeof dyn_out[i]);
        status_out[i] = rc;
        c->file_errors[i] = text;
    }
    for (size_t a = 0; a < done.size(); ++a)
        if (!done[a]) {
            memset(&albums_out[a], 0, sizeof albums_out[a]);
            if (albums_dyn_out) memset(&albums_dyn_out[a], 0, sizeof albums_dyn_out[a]);
            album_status_out[a] = rc;
        }
    c->err = text;
    return rc;
}

// =================================================================================================
extern "C" int rg_set_decoder_command(rg_ctx *c, const char *command_template) {
    if (!c) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&]() -> int {
        c->decoder_cmd = command_template ? command_template : "";
        return RG_OK;
    });
}

extern "C" int rg_analyze_wav_batch(rg_ctx *c, const void *const *wav, const size_t *wav_len, size_t n, int album,
                                    rg_track_result *out, rg_album_result *album_out) {
    if (!c) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&]() -> int {
        if (n && (!wav || !wav_len)) return rg_set_err(c, RG_ERR_INVALID_ARG, "null input array");
        std::vector<rg_track_desc> descs;
        size_t arena_bytes = 0;
        int rc = stage_wavs(c, wav, wav_len, n, &descs, &arena_bytes);
        if (rc != RG_OK) return rc;
        // the planar arena is on the device: the rest is rg_analyze_pcm_batch / rg_analyze_album_pcm, exact pass included
        if (album) return rg_analyze_album_pcm(c, descs.data(), n, c->d_arena.p, arena_bytes, 1, out, album_out, nullptr);
        return rg_analyze_pcm_batch(c, descs.data(), n, c->d_arena.p, arena_bytes, 1, out, nullptr);
    });
}

extern "C" int rg_analyze_track(rg_ctx *c, const char *path, int32_t track_index, rg_track_result *out) {
    if (!c || !out) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&]() -> int {
        rg_track_desc desc;
        size_t arena_bytes = 0;
        uint32_t file_type = 0;
        int rc = load_and_stage_one(c, path, track_index, &desc, &arena_bytes, &file_type);
        if (rc != RG_OK) return rc;
        rc = rg_analyze_pcm_batch(c, &desc, 1, c->d_arena.p, arena_bytes, 1, out, nullptr);
        if (rc != RG_OK) return rc;
        out->file_type = file_type;
        return RG_OK;
    });
}

// Files of a long list in groups whose PCM is estimated (24 bytes of planar f32 per byte of file: a 128 kb/s stereo MP3;
// denser files decode to less) to stay within a third of the free device memory, at most 64 GB.
void rgf::file_groups(rg_ctx *c, const char *const *paths, size_t n, std::vector<std::pair<size_t, size_t>> *groups) {
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
static int album_begin_impl(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *tracks_out, size_t *failed_index) {
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
    // (a status that is not a file's failure leaves *failed_index at (size_t)-1, so that a node prefers real file errors of other shares)
    for (size_t gi = 0; gi < std::max<size_t>(groups.size(), 1); ++gi) {
        const size_t first = groups.empty() ? 0 : groups[gi].first, cnt = groups.empty() ? 0 : groups[gi].second;
        FileGroup g(c, paths, first, cnt);
        const double t0 = now();
        PartsRun parts;  // album parts: one album that fits the device
        bool use_parts = false;
        rc = parts_allowed(c, cnt, groups.size(), &use_parts);
        if (rc != RG_OK) return rc;
        rc = g.load(LoadOpts{track_index}, use_parts ? &parts : nullptr);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < cnt; ++i) {
            std::string msg;
            const int frc = file_outcome(g.in[i], g.rcs[i], g.errs[i], g.paths[i], track_index, &msg);
            if (frc != RG_OK) return fail_at(first + i, rg_set_err(c, frc, "%s", msg.c_str()));
        }
        const double t1 = now();
        bool stand = false;
        rc = take_parts(c, use_parts ? &parts : nullptr, g.in, cnt, tracks_out + first, &stand);
        if (rc != RG_OK) return rc;
        if (stand) {
            rc = rg_album_parts_fold(c, parts.n_parts);
            if (rc == RG_OK && trace) fprintf(stderr, "[rg_analyze_album] load + decode + analysis in %zu parts %.1f ms, results %.1f ms\n", parts.n_parts, (t1 - t0) * 1e3, (now() - t1) * 1e3);
            return rc;
        }
        std::vector<rg_track_desc> descs;
        size_t arena_bytes = 0;
        rc = stage_loaded(c, g.in, cnt, &descs, &arena_bytes);
        if (trace) fprintf(stderr, "[rg_analyze_album] load %.1f ms, stage + device decode %.1f ms\n", (t1 - t0) * 1e3, (now() - t1) * 1e3);
        if (rc == RG_ERR_FORMAT) {  // "input i ..." -> the reference's text with the file's name
            size_t i = 0;
            if (sscanf(c->err.c_str(), "input %zu", &i) == 1 && i < cnt)
                return fail_at(first + i, rg_set_err(c, RG_ERR_FORMAT, "Failed to probe format: %s", g.paths[i]));
        }
        if (rc != RG_OK) return rc;
        const double t2 = now();
        if (groups.size() <= 1) rc = rg_album_local_pcm(c, descs.data(), cnt, c->d_arena.p, arena_bytes, 1, tracks_out);
        else rc = rg_album_part(c, descs.data(), cnt, c->d_arena.p, arena_bytes, gi, groups.size(), tracks_out + first);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < cnt; ++i) tracks_out[first + i].file_type = g.in[i].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
        if (trace) fprintf(stderr, "[rg_analyze_album] analysis %.1f ms\n", (now() - t2) * 1e3);
    }
    if (groups.size() > 1) return rg_album_parts_fold(c, groups.size());
    return RG_OK;
}

extern "C" int rg_analyze_album_begin(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *tracks_out,
                                      size_t *failed_index) {
    if (failed_index) *failed_index = (size_t)-1;
    if (!c || (n && (!paths || !tracks_out))) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&] { return album_begin_impl(c, paths, n, track_index, tracks_out, failed_index); });
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
    out += first;
    status_out += first;
    FileGroup g(c, paths, first, n);
    // parts (PartsRun), track mode: every file of the group has to come through the loader pipeline for them to count
    PartsRun parts;
    parts.album = 0;
    parts.fold = fold;
    bool use_parts = false;
    int rc = parts_allowed(c, n, 1 /* the call's other groups do not matter: tracks are independent */, &use_parts);
    if (rc != RG_OK) return rc;
    rc = g.load(LoadOpts{track_index}, use_parts ? &parts : nullptr);
    if (rc != RG_OK) return rc;
    bool stand = false;
    rc = take_parts(c, use_parts ? &parts : nullptr, g.in, n, out, &stand);
    if (rc != RG_OK) return rc;
    if (stand) {
        for (size_t i = 0; i < n; ++i) {
            status_out[i] = RG_OK;
            c->file_errors[first + i].clear();
        }
        return RG_OK;
    }
    if (fold && parts.n_parts) {  // parts were folded already: the plain route below starts the packs over
        rc = fold_init(c, fold);
        if (rc != RG_OK) return rc;
    }
    const auto mark = [&](size_t i, int code, const std::string &text) {
        memset(&out[i], 0, sizeof out[i]);
        status_out[i] = code;
        c->file_errors[first + i] = text;
    };
    // the batch holds the files that loaded and whose rate the analysis knows
    const auto screen = [&](size_t i, std::string *text) -> int {
        const int frc = file_outcome(g.in[i], RG_OK, g.errs[i], g.paths[i], track_index, text);
        if (frc != RG_OK || !fold || stageable(g.in[i])) return frc;
        *text = std::string("Failed to probe format: ") + g.paths[i];  // rg_analyze_albums: this file fails alone instead of failing every file of the batch
        return RG_ERR_FORMAT;
    };
    const auto work = [&]() -> int {
        std::vector<rg_track_result> res(g.slot.size());
        const int wrc = rg_analyze_pcm_batch(c, g.descs.data(), g.slot.size(), c->d_arena.p, g.arena_bytes, 1, res.data(), nullptr);
        if (wrc != RG_OK) return wrc;
        g.scatter(res, out);
        for (size_t k = 0; k < g.slot.size(); ++k) out[g.slot[k]].file_type = g.in[k].is_mp4 ? RG_FILE_AAC : RG_FILE_MP3;
        return RG_OK;
    };
    rc = g.run(screen, mark, work);
    if (rc != RG_OK || !g.done || !fold) return rc;
    return fold_batch(c, fold, g.slot.data(), g.slot.size(), c->slot().stream);
}

// `-r` over a whole library must not need the whole library's PCM in HBM at once: the files are taken in groups
// (file_groups).  Tracks are independent, so the groups are too.
extern "C" int rg_analyze_tracks(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, rg_track_result *out,
                                 int32_t *status_out) {
    if (!c || (n && (!paths || !out || !status_out))) return RG_ERR_INVALID_ARG;
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) { return analyze_tracks_group(c, paths, first, cnt, track_index, out, status_out); });
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
    return no_throw(c, [&]() -> int {
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
            rc = no_throw(c, [&] {
                return analyze_albums_impl(c, paths, n, album_first, n_albums, track_index, tracks_out, status_out, albums_out, album_status_out,
                                           done, &files_done);
            });
        if (rc != RG_OK) return fail_rest(c, rc, files_done, n, done, tracks_out, status_out, albums_out, album_status_out);
        return RG_OK;
    });
}

// find_peak_amplitude (src/replaygain.rs:1140-1249): max |x| over ALL channels, no loudness analysis
extern "C" int rg_find_peak_amplitude(rg_ctx *c, const char *path, rg_peak_result *out) {
    if (!c || !out) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&]() -> int {
        rg_track_desc desc;
        size_t arena_bytes = 0;
        const int rc = load_and_stage_one(c, path, -1, &desc, &arena_bytes);
        if (rc != RG_OK) return rc;
        // the arena was produced on the stream rg_find_peak_pcm uses, so no further ordering is needed
        return rg_find_peak_pcm(c, &desc, c->d_arena.p, arena_bytes, 1, out);
    });
}

// ---- EBU R 128 (include/mp3rgain_amd_r128.h): the same loaders, decoders and groups; the analysis is rg_r128.hip's ---------
// one group of files -> their results; album: the first failing file in input order aborts the call, else a failing file
// fails alone
// (kept_tr / kept_slot / kept_e, rg_r128_analyze_albums: the device descriptors of the files that were analysed, their indices in
// the group, and their hop energies in a buffer that is the caller's to free)
static int r128_files_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, int32_t track_index, int want_tp, bool album,
                            rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out /* tracks only; may be nullptr */,
                            std::vector<RgR128TrackDev> *kept_tr = nullptr, std::vector<size_t> *kept_slot = nullptr,
                            double **kept_e = nullptr) {
    out += first;
    if (dyn_out) {
        dyn_out += first;
        memset(dyn_out, 0, n * sizeof *dyn_out);
    }
    FileGroup g(c, paths, first, n);
    int rc = g.load(LoadOpts{track_index});
    if (rc != RG_OK) return rc;
    const bool layout = rg_r128_channel_mode(c) == RG_R128_CHANNELS_LAYOUT;
    const auto screen = [&](size_t i, std::string *text) -> int {
        const LoadedAudio &la = g.in[i];
        text->clear();
        const int frc = file_outcome(la, RG_OK, g.errs[i], g.paths[i], track_index, text, true);
        if (frc != RG_OK) return frc;
        if (!stageable(la)) {
            *text = std::string("Failed to probe format: ") + g.paths[i];
            return RG_ERR_FORMAT;
        }
        if (!layout) return RG_OK;
        uint32_t channels = la.channels;  // a layout has 1 to 8 channels
        if (la.kind == LoadedAudio::Wav) {
            rg_wav_info wi;
            channels = rg_wav_parse(la.wav.data(), la.wav.size(), &wi) == RG_OK ? wi.channels : 0;
        }
        if (channels >= 1 && channels <= 8) return RG_OK;
        char m[128];
        snprintf(m, sizeof m, "Unsupported channel count for layout analysis: %u (1 to 8)", channels);
        *text = m;
        return RG_ERR_INVALID_ARG;
    };
    const auto mark = [&](size_t i, int code, const std::string &text) {
        memset(&out[i], 0, sizeof out[i]);
        if (!status_out) return;  // album: the first failing file fails the call
        status_out[first + i] = code;
        c->file_errors[first + i] = text;
    };
    std::vector<rg_r128_dynamics> dyn;
    const auto work = [&]() -> int {
        const size_t k = g.slot.size();
        // LAYOUT mode: every file's weights from its container's channel mask (file j of the batch is in[j] by now)
        std::vector<rg_r128_channel_weights> weights(layout ? k : 0);
        for (size_t j = 0; j < weights.size(); ++j) {
            const uint32_t mask = g.in[j].kind == LoadedAudio::Wav ? wav_channel_mask(g.in[j].wav.data(), g.in[j].wav.size()) : 0u;
            if (rg_r128_layout_weights(g.descs[j].channels, mask, &weights[j]) != RG_OK)
                return rg_set_err(c, RG_ERR_INVALID_ARG, "Unsupported channel count for layout analysis: %u (1 to 8)", g.descs[j].channels);
        }
        std::vector<rg_r128_track_result> res(k);
        dyn.resize(dyn_out ? k : 0);
        if (kept_tr) kept_tr->resize(k);
        const int wrc = rg_r128_run(c, g.descs.data(), k, c->d_arena.p, g.arena_bytes, want_tp, album ? 1 : 0, res.data(), nullptr,
                                    dyn_out ? dyn.data() : nullptr, nullptr, kept_tr ? kept_tr->data() : nullptr, kept_e,
                                    layout ? weights.data() : nullptr);
        if (wrc == RG_OK) g.scatter(res, out);
        return wrc;
    };
    g.stop_at_first = album;
    rc = g.run(screen, mark, work);
    if (rc != RG_OK) return rc;
    if (!g.done) {  // no file for the batch, or the batch failed and its files carry that
        if (kept_tr && !g.slot.empty()) kept_tr->clear();
        return RG_OK;
    }
    if (kept_slot) *kept_slot = g.slot;
    for (size_t k = 0; k < g.slot.size() && dyn_out; ++k) dyn_out[g.slot[k]] = dyn[k];
    return RG_OK;
}

static int r128_tracks(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                       rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out) {
    if (!c || (n && (!paths || !out || !status_out))) return RG_ERR_INVALID_ARG;
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) {
        return r128_files_group(c, paths, first, cnt, track_index, want_true_peak, false, out, status_out, dyn_out);
    });
}

static int r128_album(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                      rg_r128_track_result *tracks_out, rg_r128_album_result *album_out, rg_r128_dynamics *dyn_out,
                      rg_r128_dynamics *album_dyn_out) {
    if (!c || (n && (!paths || !tracks_out)) || !album_out) return RG_ERR_INVALID_ARG;
    return no_throw(c, [&]() -> int {
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
    });
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
    if (c && n && !dyn_out) return no_throw(c, [&] { return rg_set_err(c, RG_ERR_INVALID_ARG, "null dyn_out"); });
    return r128_tracks(c, paths, n, track_index, want_true_peak, out, status_out, dyn_out);
}

extern "C" int rg_r128_analyze_album_dynamics(rg_ctx *c, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                              rg_r128_track_result *tracks_out, rg_r128_album_result *album_out,
                                              rg_r128_dynamics *dyn_out, rg_r128_dynamics *album_dyn_out) {
    if (c && ((n && !dyn_out) || !album_dyn_out)) return no_throw(c, [&] { return rg_set_err(c, RG_ERR_INVALID_ARG, "null dynamics output"); });
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
    return no_throw(c, [&]() -> int {
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
            rc = no_throw(c, [&] {
                return r128_albums_impl(c, paths, n, album_first, n_albums, track_index, want_tp, tracks_out, status_out, albums_out,
                                        album_status_out, dynamics, dyn_out, albums_dyn_out, done, &files_done, bufs);
            });
        for (const auto &b : bufs) (void)hipFree(b.second);
        if (rc != RG_OK)
            return fail_rest(c, rc, files_done, n, done, tracks_out, status_out, albums_out, album_status_out, dynamics ? dyn_out : nullptr,
                             dynamics ? albums_dyn_out : nullptr);
        return RG_OK;
    });
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
