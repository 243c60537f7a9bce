// rg_file_verify.hip -- the file-level calls that check files instead of measuring loudness: rg_flac_verify
// (include/mp3rgain_amd_flac.h), rg_mp3_verify (include/mp3rgain_amd_mp3verify.h), rg_rip_checksums
// (include/mp3rgain_amd_rip.h), and the four PCM scans, which share one group driver (pcm_scan_group): rg_pcm_stats
// (include/mp3rgain_amd_stats.h), rg_dynamic_range (include/mp3rgain_amd_dr.h), rg_ancestry (include/mp3rgain_amd_ancestry.h),
// rg_spectrum (include/mp3rgain_amd_spectrum.h), rg_same_recording (include/mp3rgain_amd_fingerprint.h), rg_tempo
// (include/mp3rgain_amd_tempo.h), rg_key (include/mp3rgain_amd_key.h) and rg_stereo (include/mp3rgain_amd_stereo.h); and the one that
// writes files, rg_flac_encode_files (include/mp3rgain_amd_flacenc.h).  They take the analysis calls' route (rg_files.h: for_each_group, FileGroup) without a decoder
// command: what this library does not decode itself is not a stream it could vouch for.  A file's status lives in its record,
// and the record of a file that failed holds nothing else.
#include <stdio.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "rg_ancestry.h"
#include "rg_clicks.h"
#include "rg_dr.h"
#include "rg_files.h"
#include "rg_flac_md5.h"
#include "rg_fprint.h"
#include "rg_mp3verify.h"
#include "rg_rip.h"
#include "rg_spectrum.h"
#include "rg_tempo.h"
#include "rg_key.h"
#include "rg_resample.h"
#include "rg_stats.h"
#include "rg_stereo.h"
#include "rg_compare.h"
#include "rg_flacenc.h"

using namespace rgf;

// "fail file i with (code, text)" where the status is the record's own: the calls zero their records before the first group
template <typename Record>
static auto mark_record(const FileGroup &g, Record *out) {
    return [&g, out](size_t i, int code, const std::string &text) {
        memset(&out[i], 0, sizeof out[i]);
        out[i].status = code;
        g.c->file_errors[g.first + i] = text;
    };
}

// ---- rg_flac_verify -------------------------------------------------------------------------------------------------------
// one group of the call: the hash of what lies in the arena (device decoder) or of the host decoder's PCM (tuning key 14 = 0),
// then the per-file records
static int flac_verify_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, rg_flac_verify_result *out) {
    out += first;
    FileGroup g(c, paths, first, n);
    int rc = g.load(LoadOpts{-1, false});
    if (rc != RG_OK) return rc;
    const auto mark = mark_record(g, out);
    const auto not_flac = [&](size_t i) { return std::string("Not a native FLAC stream: ") + g.paths[i]; };
    // everything that loaded and is not a WAV stream goes through the staging, as in an analysis call (what the loader
    // pipeline has put into the arena already stays accounted for); only the FLAC streams are hashed
    const auto screen = [&](size_t i, std::string *text) -> int {
        if (g.in[i].kind != LoadedAudio::Wav) return RG_OK;
        *text = not_flac(i);
        return RG_ERR_FORMAT;
    };
    const auto work = [&]() -> int {
        const std::vector<LoadedAudio> &in = g.in;
        std::vector<RgFlacMd5Rec> recs;
        std::vector<size_t> rec_of;  // record -> position in the batch
        for (size_t k = 0; k < g.slot.size(); ++k) {
            const size_t i = g.slot[k];
            if (in[k].kind != LoadedAudio::Flac) {
                mark(i, RG_ERR_FORMAT, not_flac(i));
                continue;
            }
            rg_flac_verify_result &r = out[i];
            rg_flac_info si;
            (void)rg_flac_scan(in[k].file_bytes.data(), in[k].file_bytes.size(), &si);  // (load_flac has walked this stream)
            if (rg_flac_stream_md5(in[k].file_bytes.data(), in[k].file_bytes.size(), r.md5_stream) == 1) r.flags |= RG_FLAC_VERIFY_HAS_SIGNATURE;
            r.frames = g.descs[k].frames;
            r.total_samples = si.total_samples;
            r.audio_frames = g.counts[k].decoded;
            r.dropped_frames = g.counts[k].dropped;
            RgFlacMd5Rec rec;
            if (in[k].flac_frames.empty()) {  // the host decoder's PCM, in the arena's format (or a stream without frames)
                rg_track_desc d = g.descs[k];
                d.offset_bytes = 0;
                const int rc = rg_flac_md5_record(c, i, d, in[k].flac_bps, in[k].flac_pcm.data(), in[k].flac_pcm.size(), &rec);
                if (rc != RG_OK) return rc;
                rg_flac_md5_host(rec, r.md5_decoded);
                continue;
            }
            const int rc = rg_flac_md5_record(c, i, g.descs[k], in[k].flac_bps, c->d_arena.p, g.arena_bytes, &rec);
            if (rc != RG_OK) return rc;
            recs.push_back(rec);
            rec_of.push_back(k);
        }
        if (!recs.empty()) {  // on the stream the decode ran on
            std::vector<uint8_t> dig(recs.size() * 16);
            const int rc = rg_flac_md5_device(c, recs.data(), recs.size(), dig.data(), c->file_stream());
            if (rc != RG_OK) return rc;
            for (size_t j = 0; j < recs.size(); ++j) memcpy(out[g.slot[rec_of[j]]].md5_decoded, &dig[16 * j], 16);
        }
        for (size_t i : g.slot) {
            rg_flac_verify_result &r = out[i];
            if (r.status != RG_OK) continue;
            if ((r.flags & RG_FLAC_VERIFY_HAS_SIGNATURE) && memcmp(r.md5_stream, r.md5_decoded, 16) == 0) r.flags |= RG_FLAC_VERIFY_MD5_MATCH;
            if (r.total_samples == 0 || r.total_samples == r.frames) r.flags |= RG_FLAC_VERIFY_LENGTH_MATCH;
            if (r.dropped_frames == 0) r.flags |= RG_FLAC_VERIFY_COMPLETE;
        }
        return RG_OK;
    };
    g.want_counts = true;
    return g.run(screen, mark, work);
}

extern "C" int rg_flac_verify(rg_ctx *c, const char *const *paths, size_t n, rg_flac_verify_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    if (n) memset(out, 0, n * sizeof *out);
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) { return flac_verify_group(c, paths, first, cnt, out); });
}

// ---- rg_mp3_verify --------------------------------------------------------------------------------------------------------
// one group of the call.  The decode side is the analysis's, so how many frames were dropped is the route's own verdict; the
// loader keeps the bytes of MPEG streams as read.  The checksums: one upload of the group's bytes with their range and frame
// tables and the kernels of rg_mp3_crc.hip, on the stream the decode ran on; with tuning key 6 = 0 (the host decoder) the host
// twin.
static int mp3_verify_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, rg_mp3_verify_result *out) {
    out += first;
    FileGroup g(c, paths, first, n);
    int rc = g.load(LoadOpts{-1, false, true});
    if (rc != RG_OK) return rc;
    const auto mark = mark_record(g, out);
    const auto not_mpeg = [&](size_t i) { return std::string("Not a bare MPEG Layer III stream: ") + g.paths[i]; };
    const auto screen = [&](size_t i, std::string *text) -> int {
        const LoadedAudio &la = g.in[i];
        const bool mpeg = la.kind == LoadedAudio::Planar || la.kind == LoadedAudio::Split || la.kind == LoadedAudio::Staged;
        if (mpeg && !la.mpeg_in_mp4) return RG_OK;
        *text = not_mpeg(i);
        return RG_ERR_FORMAT;
    };
    const auto work = [&]() -> int {
        const std::vector<LoadedAudio> &in = g.in;
        const size_t m = g.slot.size();
        std::vector<RgMp3VerifyPlan> plans(m);
        std::vector<uint32_t> dropped(m, 0);
        std::vector<char> live(m, 0);
        for (size_t k = 0; k < m; ++k) {
            const LoadedAudio &la = in[k];
            if (rg_mp3_verify_plan(la.file_bytes.data(), la.file_bytes.size(), &plans[k]) != RG_OK) {
                mark(g.slot[k], RG_ERR_FORMAT, not_mpeg(g.slot[k]));
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
            const int rc = rg_mp3_crc_device(c, job, c->file_stream());
            if (rc != RG_OK) return rc;
            for (size_t j = 0; j < f_off.size(); ++j) failed[f_of[j]] += ok[j] ? 0u : 1u;
        }
        for (size_t k = 0; k < m; ++k)
            if (live[k]) rg_mp3_verify_fill(in[k].file_bytes.data(), in[k].file_bytes.size(), plans[k], dropped[k], music[k], failed[k], &out[g.slot[k]]);
        return RG_OK;
    };
    return g.run(screen, mark, work);
}

extern "C" int rg_mp3_verify(rg_ctx *c, const char *const *paths, size_t n, rg_mp3_verify_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    if (n) memset(out, 0, n * sizeof *out);
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) { return mp3_verify_group(c, paths, first, cnt, out); });
}

// ---- rg_rip_checksums -----------------------------------------------------------------------------------------------------
// one group of the call.  The route is rg_flac_verify's, except that 16-bit stereo WAV streams are kept.  Whatever route put a
// track's PCM into the arena (device FLAC decoder, the host decoder's planes by copy, the WAV de-interleave), the two kernels
// of rg_rip_crc.hip read it there, on the stream the decode ran on, so tuning key 14 cannot show in the records.
// With `ofs` (rg_rip_offset_signatures: the group is the whole call) the batch is also taken as one disc, when every file is
// in it: the signatures at every offset of the window, from the same arena on the same stream.
struct RipOffsets {
    int32_t radius;
    uint32_t *arv1, *arv2;
};
static int rip_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const uint32_t *track_flags, rg_rip_result *out,
                     const RipOffsets *ofs = nullptr) {
    out += first;
    if (track_flags) track_flags += first;
    FileGroup g(c, paths, first, n);
    int rc = g.load(LoadOpts{-1, false});
    if (rc != RG_OK) return rc;
    const auto mark = mark_record(g, out);
    const auto refused = [&](size_t i, const std::string &why) { return "No rip checksums (" + why + "): " + g.paths[i]; };
    // everything that loaded goes through the staging, as in an analysis call (what the loader pipeline has put into the arena
    // already stays accounted for), except WAV streams that take no part: the staging cannot lay out every kind of them
    const auto screen = [&](size_t i, std::string *text) -> int {
        if (g.in[i].kind != LoadedAudio::Wav) return RG_OK;
        rg_wav_info w;
        if (rg_wav_parse(g.in[i].wav.data(), g.in[i].wav.size(), &w) != RG_OK) {
            *text = std::string("Failed to probe format: ") + g.paths[i];
            return RG_ERR_FORMAT;
        }
        if (w.sample_format == 1 && w.bits_per_sample == 16 && w.channels == 2) return RG_OK;
        *text = refused(i, std::to_string(w.channels) + " channel(s) of " + std::to_string(w.bits_per_sample) + "-bit " +
                               (w.sample_format == 3 ? "float" : "integer") + " PCM, not 2 of 16-bit integer");
        return RG_ERR_FORMAT;
    };
    const auto work = [&]() -> int {
        const std::vector<LoadedAudio> &in = g.in;
        std::vector<RgRipTrack> recs;
        std::vector<size_t> rec_of;  // record -> position in the batch
        for (size_t k = 0; k < g.slot.size(); ++k) {
            const size_t i = g.slot[k];
            if (in[k].kind != LoadedAudio::Wav && in[k].kind != LoadedAudio::Flac) {
                mark(i, RG_ERR_FORMAT, refused(i, "an MPEG stream, not a WAV or native FLAC stream"));
                continue;
            }
            if (in[k].kind == LoadedAudio::Flac && (in[k].flac_bps != 16 || in[k].channels != 2)) {
                mark(i, RG_ERR_FORMAT, refused(i, std::to_string(in[k].channels) + " channel(s) of " + std::to_string(in[k].flac_bps) + " bits per sample, not 2 of 16"));
                continue;
            }
            RgRipTrack rec;
            char err[256] = "";
            const int rc = rg_rip_track_record(i, g.descs[k], track_flags ? track_flags[i] : 0u, g.arena_bytes, &rec, err, sizeof err);
            if (rc == RG_ERR_FORMAT) {
                mark(i, RG_ERR_FORMAT, refused(i, err));
                continue;
            }
            if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
            recs.push_back(rec);
            rec_of.push_back(k);
        }
        if (recs.empty()) return RG_OK;
        std::vector<RgRipSums> sums(recs.size());
        const int rc = rg_rip_device(c, c->d_arena.p, recs.data(), recs.size(), sums.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (size_t j = 0; j < recs.size(); ++j) {
            const size_t k = rec_of[j];
            rg_rip_fill(sums[j], g.descs[k].frames, g.descs[k].sample_rate, g.counts[k].dropped, &out[g.slot[k]]);
        }
        if (!ofs || recs.size() != n) return RG_OK;  // a hole in the disc would shift every later track: no tables then
        std::vector<RgRipDiscTrack> disc(n + 1);
        rg_rip_disc(recs.data(), n, disc.data());
        return rg_rip_offsets_device(c, c->d_arena.p, disc.data(), n, ofs->radius, ofs->arv1, ofs->arv2, c->file_stream());
    };
    g.want_counts = true;
    return g.run(screen, mark, work);
}

extern "C" int rg_rip_checksums(rg_ctx *c, const char *const *paths, size_t n, const uint32_t *track_flags, rg_rip_result *out) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    if (n) memset(out, 0, n * sizeof *out);
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) { return rip_group(c, paths, first, cnt, track_flags, out); });
}

// ---- rg_rip_offset_signatures ---------------------------------------------------------------------------------------------
// rg_rip_checksums' route for one disc that lies in the arena at once, and the offsets kernel (rg_rip_offsets.hip) behind it.
extern "C" int rg_rip_offset_signatures(rg_ctx *c, const char *const *paths, size_t n, const uint32_t *track_flags, int32_t radius, rg_rip_result *out,
                                        uint32_t *arv1, uint32_t *arv2) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    if (radius < 0 || radius > RG_RIP_OFFSET_MAX) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_offset_signatures: radius %d is outside 0..%d", (int)radius, RG_RIP_OFFSET_MAX);
    if (n > RG_RIP_DISC_MAX_TRACKS) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_offset_signatures: %zu files, a disc has at most %u tracks", n, RG_RIP_DISC_MAX_TRACKS);
    const size_t table = n * (2 * (size_t)radius + 1) * sizeof(uint32_t);
    if (n) memset(out, 0, n * sizeof *out);
    if (arv1 && table) memset(arv1, 0, table);
    if (arv2 && table) memset(arv2, 0, table);
    return no_throw(c, [&]() -> int {
        c->file_errors.assign(n, std::string());
        int rc = rg_bind_device(c);
        if (rc != RG_OK || !n) return rc;
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        if (groups.size() != 1)
            return rg_set_err(c, RG_ERR_REFUSED, "No offset signatures: the %zu files would be decoded in %zu groups, and a disc must lie on the device at once", n,
                              groups.size());
        const RipOffsets ofs{radius, arv1, arv2};
        rc = rip_group(c, paths, 0, n, track_flags, out, &ofs);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i)
            if (out[i].status != RG_OK)
                return rg_set_err(c, RG_ERR_REFUSED, "No offset signatures: not every file of the disc took part: %s", c->file_errors[i].c_str());
        return RG_OK;
    });
}

// ---- the PCM scans: rg_pcm_stats, rg_dynamic_range, rg_ancestry, rg_spectrum ---------------------------------------------
// One group of such a call.  The route is rg_rip_checksums', except that every stream the library decodes itself is kept: all the
// WAV kinds the staging lays out, FLAC of any width and channel count up to 8, and MPEG Layer III as the f32 the decoder left in
// the arena.  Whatever route put a track's PCM there, the scan's kernels read it there, on the stream the decode ran on, so
// tuning key 14 cannot show in the records.  A scan is its noun ("PCM stats"), its channel limit, and two functions:
// add(k, i, err) appends the planes or views of batch entry k, file i of the group, or says why not in err[kPcmErrLen];
// finish() launches over what was added and fills the records.
constexpr size_t kPcmErrLen = 256;
namespace {
struct PcmRec {  // a track that was added, for a scan that keeps no more
    size_t k, plane;  // position in the batch, its first plane
};
}  // namespace

static std::string pcm_refused(const FileGroup &g, const char *noun, size_t i, const std::string &why) {
    return std::string("No ") + noun + " (" + why + "): " + g.paths[i];
}

// a WAV stream the staging cannot lay out, or anything of more than `max_channels` channels, fails alone and in front of the staging
static int pcm_screen(const FileGroup &g, size_t i, uint32_t max_channels, const char *noun, std::string *text) {
    uint32_t channels = g.in[i].channels;
    if (g.in[i].kind == LoadedAudio::Wav) {
        rg_wav_info w;
        if (rg_wav_parse(g.in[i].wav.data(), g.in[i].wav.size(), &w) != RG_OK) {
            *text = std::string("Failed to probe format: ") + g.paths[i];
            return RG_ERR_FORMAT;
        }
        if (wav_kind(w) < 0) {
            *text = pcm_refused(g, noun, i, std::to_string(w.bits_per_sample) + "-bit " + (w.sample_format == 3 ? "float" : "samples of format " + std::to_string(w.sample_format)) +
                                                ", not 8, 16, 24 or 32-bit integer or 32-bit float PCM");
            return RG_ERR_FORMAT;
        }
        channels = w.channels;
    }
    if (channels <= max_channels) return RG_OK;
    *text = pcm_refused(g, noun, i, std::to_string(channels) + " channels, more than " + std::to_string(max_channels));
    return RG_ERR_FORMAT;
}

// the frames the route dropped from batch entry k of a staged group (with counts): FLAC frames as the decoder counted them, MPEG
// frames as rg_mp3_verify counts them
static uint32_t dropped_frames(const FileGroup &g, size_t k) {
    const LoadedAudio &la = g.in[k];
    if (la.kind == LoadedAudio::Wav) return 0;
    if (la.kind == LoadedAudio::Flac) return g.counts[k].dropped;
    const uint32_t spf = g.descs[k].sample_rate >= 32000 ? 1152 : 576;
    return la.kind == LoadedAudio::Staged ? (uint32_t)((la.walked_frames - std::min(la.walked_frames, la.frames)) / spf) : la.mp3_skipped;
}

// `out`: the group's records.  A track add() refuses with RG_ERR_FORMAT fails alone; any other status fails the call.
template <typename Record, typename Add, typename Finish>
static int pcm_scan_group(FileGroup &g, const char *noun, uint32_t max_channels, Record *out, Add add, Finish finish) {
    const int rc = g.load(LoadOpts{-1, false});
    if (rc != RG_OK) return rc;
    const auto mark = mark_record(g, out);
    const auto screen = [&](size_t i, std::string *text) { return pcm_screen(g, i, max_channels, noun, text); };
    const auto work = [&]() -> int {
        for (size_t k = 0; k < g.slot.size(); ++k) {
            const size_t i = g.slot[k];
            char err[kPcmErrLen] = "";
            const int prc = add(k, i, err);
            if (prc == RG_ERR_FORMAT)
                mark(i, RG_ERR_FORMAT, pcm_refused(g, noun, i, err));
            else if (prc != RG_OK)
                return rg_set_err(g.c, prc, "%s", err);
        }
        return finish();
    };
    g.want_counts = true;
    return g.run(screen, mark, work);
}

// the call around the groups: the options checked by `options`, the records (and `also`, when there is one) zeroed, then
// group(first, cnt, o) for each group of the list
template <typename Opts, typename Record, typename Options, typename Group>
static int pcm_scan_call(rg_ctx *c, const char *const *paths, size_t n, const Opts *opts, Record *out, Options options, Group group, void *also = nullptr,
                         size_t also_bytes = 0) {
    if (!c || (n && (!paths || !out))) return RG_ERR_INVALID_ARG;
    Opts o;
    char err[256] = "";
    const int orc = options(opts, &o, err, sizeof err);
    if (orc != RG_OK) return rg_set_err(c, orc, "%s", err);
    if (n) memset(out, 0, n * sizeof *out);
    if (also && also_bytes) memset(also, 0, also_bytes);
    return for_each_group(c, paths, n, [&](size_t first, size_t cnt) { return group(first, cnt, o); });
}

// ---- rg_pcm_stats: the two kernels of rg_stats.hip ------------------------------------------------------------------------
static int stats_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_pcm_stats_opts &o, rg_pcm_stats_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    struct Rec {
        size_t k, plane;  // position in the batch, its first plane
        uint32_t bits;    // as the record reports them
    };
    std::vector<Rec> recs;
    std::vector<RgStatsPlane> planes(n * RG_STATS_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const LoadedAudio &la = g.in[k];
        uint32_t bits = rg_pcm_width(g.descs[k].format);
        if (la.kind == LoadedAudio::Wav) {
            rg_wav_info w;
            (void)rg_wav_parse(la.wav.data(), la.wav.size(), &w);  // (the screen has parsed this stream)
            bits = w.bits_per_sample;
        } else if (la.kind == LoadedAudio::Flac) {
            bits = la.flac_bps;
        }
        Rec r{k, n_planes, 0};
        const int rc = rg_stats_track_planes(i, g.descs[k], bits, g.arena_bytes, &planes[n_planes], &r.bits, err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(r);
        n_planes += g.descs[k].channels;
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<rg_pcm_stats_channel> ch(n_planes);
        const int rc = rg_stats_device(c, c->d_arena.p, planes.data(), n_planes, o, ch.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (const Rec &r : recs) rg_stats_fill(g.descs[r.k], r.bits, dropped_frames(g, r.k), &ch[r.plane], &out[g.slot[r.k]]);
        return RG_OK;
    };
    return pcm_scan_group(g, "PCM stats", RG_STATS_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_pcm_stats(rg_ctx *c, const char *const *paths, size_t n, const rg_pcm_stats_opts *opts, rg_pcm_stats_result *out) {
    return pcm_scan_call(c, paths, n, opts, out, rg_stats_options,
                         [&](size_t first, size_t cnt, const rg_pcm_stats_opts &o) { return stats_group(c, paths, first, cnt, o, out); });
}

// ---- rg_dynamic_range: the kernels of rg_dr.hip; the finish is host arithmetic on what comes back (rg_dr_fill) -------------
static int dr_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_dr_opts &o, rg_dr_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    std::vector<PcmRec> recs;
    std::vector<RgDrPlane> planes(n * RG_DR_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_dr_track_planes(i, g.descs[k], o, true, g.arena_bytes, &planes[n_planes], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, n_planes});
        n_planes += g.descs[k].channels;
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<RgDrPlaneOut> po(n_planes);
        const int rc = rg_dr_device(c, c->d_arena.p, planes.data(), n_planes, po.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (const PcmRec &r : recs) rg_dr_fill(g.descs[r.k], planes[r.plane].block, dropped_frames(g, r.k), &po[r.plane], &out[g.slot[r.k]]);
        return RG_OK;
    };
    return pcm_scan_group(g, "dynamic range", RG_DR_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_dynamic_range(rg_ctx *c, const char *const *paths, size_t n, const rg_dr_opts *opts, rg_dr_result *out) {
    return pcm_scan_call(c, paths, n, opts, out, rg_dr_options, [&](size_t first, size_t cnt, const rg_dr_opts &o) { return dr_group(c, paths, first, cnt, o, out); });
}

// ---- rg_stereo: the kernels of rg_stereo.hip; the finish is host arithmetic on what comes back (rg_st_fill) ------------------
// The caller's lag sums are rows by file, so a group fills the rows of its own files.
static int stereo_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_stereo_opts &o, rg_stereo_result *out, int64_t *lag_sums) {
    FileGroup g(c, paths, first, n);
    out += first;
    const uint32_t W = 2u * o.radius + 1u;
    std::vector<PcmRec> recs;  // plane: the track's place in `tracks`
    std::vector<RgStTrack> tracks(n + 1);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_st_track(i, g.descs[k], o, true, g.arena_bytes, &tracks[recs.size()], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, recs.size()});
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<RgStTotals> tot(recs.size());
        std::vector<int64_t> sums(lag_sums ? recs.size() * W : 0);
        const int rc = rg_st_device(c, c->d_arena.p, tracks.data(), recs.size(), o.radius, tot.data(), lag_sums ? sums.data() : nullptr, c->file_stream());
        if (rc != RG_OK) return rc;
        for (const PcmRec &r : recs) {
            rg_st_fill(g.descs[r.k], o, tracks[r.plane].block, dropped_frames(g, r.k), tot[r.plane], &out[g.slot[r.k]]);
            if (lag_sums) memcpy(lag_sums + (first + g.slot[r.k]) * W, &sums[r.plane * W], W * sizeof(int64_t));
        }
        return RG_OK;
    };
    return pcm_scan_group(g, "stereo scan", RG_ST_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_stereo(rg_ctx *c, const char *const *paths, size_t n, const rg_stereo_opts *opts, rg_stereo_result *out, int64_t *lag_sums) {
    rg_stereo_opts probe;
    char err[8];
    const size_t rows = rg_st_options(opts, &probe, err, sizeof err) == RG_OK ? n * (2u * probe.radius + 1u) * sizeof(int64_t) : 0;  // (pcm_scan_call reports a bad option)
    return pcm_scan_call(
        c, paths, n, opts, out, rg_st_options, [&](size_t first, size_t cnt, const rg_stereo_opts &o) { return stereo_group(c, paths, first, cnt, o, out, lag_sums); },
        lag_sums, rows);
}

// ---- rg_flac_encode_files: the kernels of rg_flacenc.hip; the metadata and the files are host work ---------------------------
static bool same_file(const char *a, const char *b) {
    struct stat sa, sb;
    return stat(a, &sa) == 0 && stat(b, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

// `bytes` into "<path>.part", then linked to `path`: a file that exists is never replaced, and no partial file is left
static bool write_new_file(const char *path, const uint8_t *bytes, size_t len, std::string *why) {
    const std::string part = std::string(path) + ".part";
    FILE *f = fopen(part.c_str(), "wb");
    if (!f) {
        *why = std::string("cannot create ") + part;
        return false;
    }
    const bool wrote = fwrite(bytes, 1, len, f) == len;
    const bool closed = fclose(f) == 0;
    bool ok = wrote && closed;
    if (!ok) *why = std::string("cannot write ") + part;
    if (ok && link(part.c_str(), path) != 0) {
        ok = false;
        *why = std::string("cannot name the output (it exists?): ") + path;
    }
    (void)unlink(part.c_str());
    return ok;
}

static int flac_encode_group(rg_ctx *c, const char *const *paths, const char *const *out_paths, size_t first, size_t n, uint32_t block, uint32_t max_lpc,
                             uint32_t flags, rg_flac_encode_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    out_paths += first;
    const int lrc = g.load(LoadOpts{-1, false});
    if (lrc != RG_OK) return lrc;
    const auto mark = mark_record(g, out);
    const auto screen = [&](size_t i, std::string *text) -> int {
        const LoadedAudio &la = g.in[i];
        if (la.kind != LoadedAudio::Wav && la.kind != LoadedAudio::Flac) {
            *text = pcm_refused(g, "FLAC encode", i, "an MPEG source: a lossless container round lossy audio");
            return RG_ERR_FORMAT;
        }
        const int rc = pcm_screen(g, i, 8, "FLAC encode", text);
        if (rc != RG_OK) return rc;
        if (la.kind == LoadedAudio::Wav) {
            rg_wav_info w;
            (void)rg_wav_parse(la.wav.data(), la.wav.size(), &w);  // (pcm_screen has parsed this stream)
            if (w.sample_format == 3 || w.bits_per_sample > 24) {
                *text = pcm_refused(g, "FLAC encode", i, w.sample_format == 3 ? "float samples" : "32-bit samples, more than 24");
                return RG_ERR_FORMAT;
            }
        }
        struct stat sb;
        if (!out_paths[i] || !*out_paths[i]) {
            *text = std::string("No output path for: ") + g.paths[i];
            return RG_ERR_IO;
        }
        if (same_file(g.paths[i], out_paths[i])) {
            *text = std::string("The output is the input: ") + out_paths[i];
            return RG_ERR_IO;
        }
        if (lstat(out_paths[i], &sb) == 0) {
            *text = std::string("The output exists: ") + out_paths[i];
            return RG_ERR_IO;
        }
        return RG_OK;
    };
    const auto work = [&]() -> int {
        std::vector<RgFeStream> st;
        std::vector<std::vector<uint8_t>> blocks;
        std::vector<size_t> ks;  // stream -> position in the batch
        for (size_t k = 0; k < g.slot.size(); ++k) {
            const size_t i = g.slot[k];
            const LoadedAudio &la = g.in[k];
            uint32_t bps = la.flac_bps;
            if (la.kind == LoadedAudio::Wav) {
                rg_wav_info w;
                (void)rg_wav_parse(la.wav.data(), la.wav.size(), &w);
                bps = w.bits_per_sample;
            }
            char err[kPcmErrLen] = "";
            RgFeStream s;
            const int rc = rg_fe_stream(i, g.descs[k], bps, c->d_arena.p, g.arena_bytes, block, max_lpc, &s, err, sizeof err);
            if (rc == RG_ERR_FORMAT) {
                mark(i, rc, pcm_refused(g, "FLAC encode", i, err));
                continue;
            }
            if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
            std::vector<uint8_t> b;
            if (la.kind == LoadedAudio::Flac && rg_fe_source_blocks(la.file_bytes.data(), la.file_bytes.size(), &b)) s.meta_bytes = (uint32_t)(42 + b.size());
            else b.clear();  // the vendor block
            st.push_back(s);
            blocks.push_back(std::move(b));
            ks.push_back(k);
        }
        if (st.empty()) return RG_OK;
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> offsets(st.size() + 1);
        std::vector<rg_flac_encode_result> res(st.size());
        int rc = rg_fe_device(c, st, &blocks, nullptr, 0, &bytes, offsets.data(), res.data(), c->file_stream(), nullptr);
        if (rc != RG_OK) return rc;
        std::vector<uint8_t> ok(st.size(), 1);
        if (flags & RG_FLAC_ENC_VERIFY) {
            rc = rg_fe_verify_device(c, st, bytes.data(), offsets.data(), res.data(), &ok, c->file_stream());
            if (rc != RG_OK) return rc;
        }
        for (size_t j = 0; j < st.size(); ++j) {
            const size_t k = ks[j], i = g.slot[k];
            rg_flac_encode_result r = res[j];
            r.dropped_frames = dropped_frames(g, k);
            if (r.dropped_frames) r.flags &= ~RG_FLAC_ENC_COMPLETE;
            if (!ok[j]) {
                mark(i, RG_ERR_STATE, std::string("The encoded stream does not decode to its source (nothing was written): ") + g.paths[i]);
                out[i].flags = RG_FLAC_ENC_VERIFY_FAILED;
                continue;
            }
            if (flags & RG_FLAC_ENC_VERIFY) r.flags |= RG_FLAC_ENC_VERIFIED;
            std::string why;
            if (!write_new_file(out_paths[i], bytes.data() + offsets[j], (size_t)(offsets[j + 1] - offsets[j]), &why)) {
                mark(i, RG_ERR_IO, why);
                continue;
            }
            r.flags |= RG_FLAC_ENC_WRITTEN;
            out[i] = r;
        }
        return RG_OK;
    };
    g.want_counts = true;
    return g.run(screen, mark, work);
}

extern "C" int rg_flac_encode_files(rg_ctx *c, const char *const *in_paths, const char *const *out_paths, size_t n, const rg_flac_encode_options *options,
                                    rg_flac_encode_result *results) {
    if (!c || (n && (!in_paths || !out_paths || !results))) return RG_ERR_INVALID_ARG;
    uint32_t block, max_lpc, flags;
    char err[256] = "";
    const int orc = rg_fe_options(options, &block, &max_lpc, &flags, err, sizeof err);
    if (orc != RG_OK) return rg_set_err(c, orc, "%s", err);
    if (n) memset(results, 0, n * sizeof *results);
    return for_each_group(c, in_paths, n, [&](size_t first, size_t cnt) { return flac_encode_group(c, in_paths, out_paths, first, cnt, block, max_lpc, flags, results); });
}

// ---- rg_clicks: the kernels of rg_clicks.hip; the channel records and the merge of the planes' event lists are host code (rg_ck_fill)
// The caller's event list is rows by file, so a group fills the rows of its own files.
static int clicks_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_clicks_opts &o, rg_clicks_result *out, rg_clicks_event *events) {
    FileGroup g(c, paths, first, n);
    out += first;
    const uint32_t K = o.max_events;
    std::vector<PcmRec> recs;
    std::vector<RgCkPlane> planes(n * RG_CK_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_ck_track_planes(i, g.descs[k], o, g.arena_bytes, &planes[n_planes], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, n_planes});
        n_planes += g.descs[k].channels;
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<RgCkTile> po(n_planes);
        std::vector<RgCkEv> ev(n_planes * K + 1);
        const int rc = rg_ck_device(c, c->d_arena.p, planes.data(), n_planes, o, po.data(), ev.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (const PcmRec &r : recs)
            rg_ck_fill(g.descs[r.k], o, dropped_frames(g, r.k), &po[r.plane], &ev[r.plane * K], &out[g.slot[r.k]], events ? events + (first + g.slot[r.k]) * K : nullptr);
        return RG_OK;
    };
    return pcm_scan_group(g, "click scan", RG_CK_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_clicks(rg_ctx *c, const char *const *paths, size_t n, const rg_clicks_opts *opts, rg_clicks_result *out, rg_clicks_event *events) {
    rg_clicks_opts probe;
    char err[8];
    const size_t rows = rg_ck_options(opts, &probe, err, sizeof err) == RG_OK ? n * probe.max_events * sizeof(rg_clicks_event) : 0;  // (pcm_scan_call reports a bad option)
    return pcm_scan_call(
        c, paths, n, opts, out, rg_ck_options, [&](size_t first, size_t cnt, const rg_clicks_opts &o) { return clicks_group(c, paths, first, cnt, o, out, events); },
        events, rows);
}

// ---- rg_ancestry: the kernels of rg_ancestry.hip; the verdict is host arithmetic on the counts that come back (rg_anc_fill) --
static int ancestry_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_ancestry_opts &o, rg_ancestry_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    struct Rec {
        size_t k, view;  // position in the batch, its first view
        uint32_t n_views, S, G;
    };
    std::vector<Rec> recs;
    std::vector<RgAncView> views(n * RG_ANC_MAX_VIEWS + 1);
    std::vector<RgAncJob> jobs;
    size_t n_views = 0;
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        Rec r{k, n_views, 0, 0, 0};
        const int rc = rg_anc_track_views(i, g.descs[k], g.arena_bytes, &views[n_views], &r.n_views, err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        for (uint32_t v = 0; v < r.n_views; ++v) rg_anc_jobs(g.descs[k].frames, o, (uint32_t)(n_views + v), &jobs, &r.S, &r.G);
        recs.push_back(r);
        n_views += r.n_views;
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        const size_t per_view = 2 * RG_ANC_ALIGNMENTS;
        std::vector<uint64_t> cnt(n_views * per_view), nonfinite(n_views);
        const int rc = rg_anc_device(c, c->d_arena.p, views.data(), n_views, jobs, o.active_floor, cnt.data(), nonfinite.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (const Rec &r : recs)
            rg_anc_fill(g.descs[r.k], o, r.S, r.G, dropped_frames(g, r.k), r.n_views, &views[r.view], &cnt[r.view * per_view], &nonfinite[r.view],
                        &out[g.slot[r.k]]);
        return RG_OK;
    };
    return pcm_scan_group(g, "ancestry scan", RG_ANC_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_ancestry(rg_ctx *c, const char *const *paths, size_t n, const rg_ancestry_opts *opts, rg_ancestry_result *out) {
    return pcm_scan_call(c, paths, n, opts, out, rg_anc_options,
                         [&](size_t first, size_t cnt, const rg_ancestry_opts &o) { return ancestry_group(c, paths, first, cnt, o, out); });
}

// ---- rg_spectrum: the two kernels of rg_spectrum.hip; the verdict is host arithmetic on what comes back (rg_spec_fill) -------
static int spectrum_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_spectrum_opts &o, rg_spectrum_result *out, double *bands) {
    const size_t per_file = RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS;
    FileGroup g(c, paths, first, n);
    out += first;
    if (bands) bands += first * per_file;
    std::vector<PcmRec> recs;
    std::vector<RgSpecPlane> planes(n * RG_SPEC_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_spec_track_planes(i, g.descs[k], g.arena_bytes, &planes[n_planes], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, n_planes});
        n_planes += g.descs[k].channels;
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<RgSpecPlaneOut> po(n_planes);
        const int rc = rg_spectrum_device(c, c->d_arena.p, planes.data(), n_planes, po.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        for (const PcmRec &r : recs)
            rg_spec_fill(g.descs[r.k], dropped_frames(g, r.k), &po[r.plane], o, &out[g.slot[r.k]], bands ? bands + g.slot[r.k] * per_file : nullptr);
        return RG_OK;
    };
    return pcm_scan_group(g, "spectrum", RG_SPEC_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_spectrum(rg_ctx *c, const char *const *paths, size_t n, const rg_spectrum_opts *opts, rg_spectrum_result *out, double *bands_out) {
    return pcm_scan_call(
        c, paths, n, opts, out, rg_spec_options,
        [&](size_t first, size_t cnt, const rg_spectrum_opts &o) { return spectrum_group(c, paths, first, cnt, o, out, bands_out); }, bands_out,
        n * RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS * sizeof(double));
}


// ---- rg_same_recording: the fingerprint kernels of rg_fprint.hip per group, the match kernel of rg_fprint_match.hip once ----
// The codes of every group stay in c->d_fp_codes, one group's behind the other's; `used` counts them.
namespace {
struct FpCall {
    size_t used = 0;  // codes in c->d_fp_codes
};
}  // namespace

// room for `need` codes with the first `used` kept
static int fp_codes_grow(rg_ctx *c, size_t used, size_t need, hipStream_t s) {
    if (need <= c->d_fp_codes.cap) return RG_OK;
    DevBuf<uint32_t> bigger;
    RG_HIP(c, bigger.reserve(std::max(need, 2 * c->d_fp_codes.cap)));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(bigger.p, c->d_fp_codes.p, used * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        bigger.release();
        RG_HIP(c, e);
    }
    c->d_fp_codes.release();
    c->d_fp_codes = bigger;
    return RG_OK;
}

static int fingerprint_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, FpCall *call, rg_fingerprint_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    std::vector<PcmRec> recs;  // plane: the track's place in `tracks`
    std::vector<RgFpTrack> tracks(n + 1);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_fp_track(i, g.descs[k], g.arena_bytes, &tracks[recs.size()], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, recs.size()});
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        uint64_t fmt_tile[4], codes = 0;
        (void)rg_fp_plan(tracks.data(), recs.size(), fmt_tile, call->used, 0);
        for (size_t t = 0; t < recs.size(); ++t) codes += tracks[t].frames ? tracks[t].frames - 1u : 0u;
        int rc = fp_codes_grow(c, call->used, call->used + (size_t)codes + 4, c->file_stream());
        if (rc != RG_OK) return rc;
        std::vector<uint32_t> nonfinite(recs.size());
        rc = rg_fprint_device(c, c->d_arena.p, tracks.data(), recs.size(), c->d_fp_codes.p, nullptr, nonfinite.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        call->used += (size_t)codes;
        for (const PcmRec &r : recs)
            rg_fp_fill(g.descs[r.k], tracks[r.plane], dropped_frames(g, r.k), nonfinite[r.plane], (uint32_t)(first + g.slot[r.k]), &out[g.slot[r.k]]);
        return RG_OK;
    };
    return pcm_scan_group(g, "fingerprint", RG_FP_MAX_CHANNELS, out, add, finish);
}

// what follows the last group of rg_same_recording and of rg_same_recording_xrate: the pair list, the match kernel over the
// `used` codes in c->d_fp_codes, the groups, the caller's pairs and its copy of the codes
static int fp_match_call(rg_ctx *c, size_t n, const std::vector<uint32_t> &counts, const std::vector<uint32_t> &rates, const std::vector<uint64_t> &at,
                         const rg_fingerprint_opts &o, size_t used, rg_fingerprint_pair *pairs, size_t max_pairs, size_t *n_pairs, uint32_t *codes_out,
                         size_t codes_cap, std::vector<uint32_t> *groups, std::vector<uint32_t> *matches) {
    hipStream_t s = c->file_stream();
    groups->assign(n, 0);
    matches->assign(n, 0);
    std::vector<rg_fingerprint_pair_record> records(n * (n - 1) / 2 + 1);
    std::vector<RgFpPair> compared;
    rg_fp_pairs(n, counts.data(), rates.data(), at.data(), o, &compared, records.data());
    const int mrc = rg_fprint_match_device(c, c->d_fp_codes.p, compared, o, records.data(), s);
    if (mrc != RG_OK) return mrc;
    *n_pairs = rg_fingerprint_groups(n, records.data(), groups->data(), matches->data());
    size_t rec = 0, found = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j, ++rec) {
            const rg_fingerprint_pair_record &r = records[rec];
            if (!(r.flags & RG_FP_PAIR_MATCH)) continue;
            if (found < max_pairs) pairs[found] = rg_fingerprint_pair{(uint32_t)i, (uint32_t)j, r.errors, r.bits, r.lag, r.flags};
            ++found;
        }
    const size_t fit = std::min(used, codes_cap);
    if (fit) {
        RG_HIP(c, hipMemcpyAsync(codes_out, c->d_fp_codes.p, fit * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
    }
    return RG_OK;
}

extern "C" int rg_same_recording(rg_ctx *c, const char *const *paths, size_t n, const rg_fingerprint_opts *opts, rg_fingerprint_result *out,
                                 rg_fingerprint_pair *pairs, size_t max_pairs, size_t *n_pairs, uint32_t *codes_out, size_t codes_cap) {
    if (!c || !n_pairs || (max_pairs && !pairs) || (codes_cap && !codes_out)) return RG_ERR_INVALID_ARG;
    *n_pairs = 0;
    if (n > 65535) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_same_recording: %zu files, at most 65535 in one call", n);
    FpCall call;
    rg_fingerprint_opts o;
    int rc = pcm_scan_call(c, paths, n, opts, out, rg_fp_options,
                           [&](size_t first, size_t cnt, const rg_fingerprint_opts &) { return fingerprint_group(c, paths, first, cnt, &call, out); });
    if (rc != RG_OK || n == 0) return rc;
    char err[256] = "";
    (void)rg_fp_options(opts, &o, err, sizeof err);  // (the call above has checked them)
    return no_throw(c, [&]() -> int {
        std::vector<uint32_t> counts(n), rates(n);
        std::vector<uint64_t> at(n);
        for (size_t i = 0; i < n; ++i) {  // a failing file has no codes and takes part in no pair
            const bool ok = out[i].status == RG_OK;
            counts[i] = ok ? out[i].codes : 0u;
            rates[i] = ok ? out[i].sample_rate : 0u;
            at[i] = ok ? out[i].codes_at : 0u;
        }
        std::vector<uint32_t> groups, matches;
        const int mrc = fp_match_call(c, n, counts, rates, at, o, call.used, pairs, max_pairs, n_pairs, codes_out, codes_cap, &groups, &matches);
        if (mrc != RG_OK) return mrc;
        for (size_t i = 0; i < n; ++i) {
            if (out[i].status != RG_OK) continue;
            out[i].group = groups[i];
            out[i].matches = matches[i];
            if (!codes_out || out[i].codes_at + out[i].codes > codes_cap) out[i].codes_at = UINT64_MAX;
        }
        return RG_OK;
    });
}

// ---- rg_compare: the fingerprint kernels and the match kernel for the coarse hints of the requested pairs, then the kernels of
// rg_compare.hip; the pick and the finish are host arithmetic on what comes back (rg_cmp_pick, rg_cmp_fill) ----------------------
// The unit of work is a pair, and both files of a pair must lie in the arena together: the whole list is one group.
namespace {
struct CmpFile {  // what mark_record takes: a file that fails, fails its pairs
    int32_t status;
};
}  // namespace

// the coarse hints of the pairs whose files both loaded: hints[p] <- 512 * lag, brought to "b behind a"; coarse[p] <- 0 when the
// match skipped the pair
static int compare_coarse(rg_ctx *c, const FileGroup &g, const std::vector<rg_track_desc> &fdesc, const std::vector<char> &loaded, const rg_compare_pair *pairs,
                          size_t n_pairs, const rg_compare_opts &o, std::vector<int64_t> *hints, std::vector<char> *coarse) {
    const size_t n = fdesc.size();
    std::vector<RgFpTrack> tracks(n + 1);
    std::vector<size_t> track_of(n, SIZE_MAX);
    size_t m = 0;
    char err[kPcmErrLen] = "";
    for (size_t i = 0; i < n; ++i) {
        if (!loaded[i]) continue;
        const int rc = rg_fp_track(i, fdesc[i], g.arena_bytes, &tracks[m], err, sizeof err);
        if (rc == RG_ERR_FORMAT) continue;  // no fingerprint of this file: its pairs get no coarse hint
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
        track_of[i] = m++;
    }
    if (!m) return RG_OK;
    uint64_t fmt_tile[4], codes = 0;
    (void)rg_fp_plan(tracks.data(), m, fmt_tile, 0, 0);
    for (size_t t = 0; t < m; ++t) codes += tracks[t].frames ? tracks[t].frames - 1u : 0u;
    int rc = fp_codes_grow(c, 0, (size_t)codes + 4, c->file_stream());
    if (rc != RG_OK) return rc;
    std::vector<uint32_t> nonfinite(m);
    rc = rg_fprint_device(c, c->d_arena.p, tracks.data(), m, c->d_fp_codes.p, nullptr, nonfinite.data(), c->file_stream());
    if (rc != RG_OK) return rc;
    rg_fingerprint_opts fo;
    (void)rg_fp_options(nullptr, &fo, err, sizeof err);
    fo.radius = o.coarse_radius;
    std::vector<RgFpPair> compared;
    std::vector<rg_fingerprint_pair_record> records(n_pairs + 1, rg_fingerprint_pair_record{0u, 0u, 0, RG_FP_PAIR_SKIPPED});
    std::vector<char> probe_b(n_pairs, 0);
    for (size_t p = 0; p < n_pairs; ++p) {
        const size_t ta = track_of[pairs[p].a], tb = track_of[pairs[p].b];
        if (ta == SIZE_MAX || tb == SIZE_MAX || fdesc[pairs[p].a].sample_rate != fdesc[pairs[p].b].sample_rate) continue;
        const RgFpTrack &A = tracks[ta], &B = tracks[tb];
        const uint32_t ka = A.frames ? A.frames - 1u : 0u, kb = B.frames ? B.frames - 1u : 0u;
        if (!A.rate_ok || !B.rate_ok || ka < fo.block || kb < fo.block) continue;
        probe_b[p] = kb < ka;  // the probe side is the one with fewer codes, on a tie the reference copy
        compared.push_back(probe_b[p] ? RgFpPair{B.codes_at, A.codes_at, kb, ka, (uint32_t)p, RG_FP_PAIR_COMPARED | RG_FP_PAIR_PROBE_J}
                                      : RgFpPair{A.codes_at, B.codes_at, ka, kb, (uint32_t)p, RG_FP_PAIR_COMPARED});
    }
    if (!compared.empty()) {
        rc = rg_fprint_match_device(c, c->d_fp_codes.p, compared, fo, records.data(), c->file_stream());
        if (rc != RG_OK) return rc;
    }
    for (size_t p = 0; p < n_pairs; ++p) {
        if ((records[p].flags & RG_FP_PAIR_SKIPPED) || !records[p].bits) continue;
        (*coarse)[p] = 1;
        (*hints)[p] = (int64_t)RG_FP_HOP * records[p].lag * (probe_b[p] ? -1 : 1);
    }
    return RG_OK;
}

static int compare_group(rg_ctx *c, const char *const *paths, size_t n, const rg_compare_pair *pairs, size_t n_pairs, const rg_compare_opts &o,
                         rg_compare_result *out, rg_compare_block *blocks_out, size_t blocks_per_pair, int64_t *lag_sums) {
    FileGroup g(c, paths, 0, n);
    std::vector<CmpFile> files(n + 1);
    std::vector<rg_track_desc> fdesc(n);
    std::vector<char> loaded(n, 0);
    std::vector<uint32_t> dropped(n, 0);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_pcm_check_format(i, g.descs[k], RG_CMP_MAX_CHANNELS, "the null test takes", err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        fdesc[i] = g.descs[k];
        loaded[i] = 1;
        dropped[i] = dropped_frames(g, k);
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        std::vector<int64_t> hints(n_pairs, 0);
        std::vector<char> coarse(n_pairs, 0);
        if (o.align == RG_CMP_ALIGN_HINT) {
            for (size_t p = 0; p < n_pairs; ++p) hints[p] = pairs[p].hint;
        } else {
            const int rc = compare_coarse(c, g, fdesc, loaded, pairs, n_pairs, o, &hints, &coarse);
            if (rc != RG_OK) return rc;
        }
        std::vector<RgCmpPair> plan;
        std::vector<size_t> pair_of;
        std::vector<rg_compare_pair> hinted(n_pairs);
        char err[kPcmErrLen] = "";
        for (size_t p = 0; p < n_pairs; ++p) {
            hinted[p] = rg_compare_pair{pairs[p].a, pairs[p].b, hints[p]};
            if (!loaded[pairs[p].a] || !loaded[pairs[p].b]) continue;  // (the record has the failing file's status)
            RgCmpPair rec;
            const int rc = rg_cmp_plan_pair(p, fdesc.data(), n, hinted[p], o, true, g.arena_bytes, &rec, err, sizeof err);
            if (rc == RG_ERR_FORMAT) {
                out[p].status = RG_ERR_FORMAT;
                c->pair_errors[p] = std::string("No comparison (") + err + "): " + g.paths[pairs[p].a] + " against " + g.paths[pairs[p].b];
                continue;
            }
            if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
            plan.push_back(rec);
            pair_of.push_back(p);
        }
        const size_t m = plan.size();
        std::vector<RgCmpPicked> picked(m + 1);
        std::vector<RgCmpTotals> tot(m + 1);
        std::vector<int64_t> rows;
        std::vector<rg_compare_block> blocks;
        const int rc = rg_cmp_device(c, c->d_arena.p, plan.data(), m, o, &rows, picked.data(), tot.data(), &blocks, c->file_stream());
        if (rc != RG_OK) return rc;
        const size_t slab = (size_t)o.segments * RG_CMP_MAX_CHANNELS * rg_cmp_row_len(o.radius);
        for (size_t j = 0; j < m; ++j) {
            const size_t p = pair_of[j];
            const RgCmpPair &r = plan[j];
            const uint32_t da = dropped[pairs[p].a], db = dropped[pairs[p].b];
            const uint32_t more = (o.align != RG_CMP_ALIGN_HINT && !coarse[p]) ? RG_CMP_NO_COARSE : 0u;
            if (!r.cc) {
                rg_cmp_fill_skipped(fdesc.data(), hinted[p], o, r, da, db, &out[p]);
                if (!(r.flags & RG_CMP_RATE)) out[p].flags |= more;  // (another rate: nothing was looked for)
                continue;
            }
            const rg_compare_block *mine = blocks.data() + r.first_block;
            rg_cmp_fill(fdesc.data(), hinted[p], o, r, picked[j], tot[j], mine, da, db, more, &out[p]);
            if (lag_sums) rg_cmp_rows_out(r, o, rows.data() + r.first_row * rg_cmp_row_len(o.radius), lag_sums + p * slab);
            if (blocks_out) rg_cmp_blocks_out(r, mine, blocks_out + p * blocks_per_pair, blocks_per_pair);
        }
        return RG_OK;
    };
    const int rc = pcm_scan_group(g, "comparison", RG_CMP_MAX_CHANNELS, files.data(), add, finish);
    if (rc != RG_OK) return rc;
    for (size_t p = 0; p < n_pairs; ++p)  // a failing file fails its own pairs only: the record zero apart from `status`
        for (const uint32_t i : {pairs[p].a, pairs[p].b})
            if (files[i].status != RG_OK && out[p].status == RG_OK) {
                memset(&out[p], 0, sizeof out[p]);
                out[p].status = files[i].status;
            }
    return RG_OK;
}

extern "C" int rg_compare(rg_ctx *c, const char *const *paths, size_t n, const rg_compare_pair *pairs, size_t n_pairs, const rg_compare_opts *opts,
                          rg_compare_result *out, rg_compare_block *blocks_out, size_t blocks_per_pair, int64_t *lag_sums) {
    if (!c || (n && !paths) || (n_pairs && (!pairs || !out))) return RG_ERR_INVALID_ARG;
    rg_compare_opts o;
    char err[256] = "";
    const int orc = rg_cmp_options(opts, &o, err, sizeof err);
    if (orc != RG_OK) return rg_set_err(c, orc, "%s", err);
    for (size_t p = 0; p < n_pairs; ++p) {
        if (pairs[p].a >= n || pairs[p].b >= n) return rg_set_err(c, RG_ERR_INVALID_ARG, "pair %zu: (%u, %u) is not a pair of the %zu files", p, pairs[p].a, pairs[p].b, n);
        if (pairs[p].a == pairs[p].b) return rg_set_err(c, RG_ERR_INVALID_ARG, "pair %zu: file %u against itself", p, pairs[p].a);
        if (pairs[p].hint > RG_CMP_MAX_HINT || pairs[p].hint < -RG_CMP_MAX_HINT)
            return rg_set_err(c, RG_ERR_INVALID_ARG, "pair %zu: a hint of %lld frames is beyond 2^32", p, (long long)pairs[p].hint);
    }
    if (n_pairs) memset(out, 0, n_pairs * sizeof *out);
    const size_t slab = (size_t)o.segments * RG_CMP_MAX_CHANNELS * rg_cmp_row_len(o.radius);
    if (lag_sums && n_pairs) memset(lag_sums, 0, n_pairs * slab * sizeof(int64_t));
    if (blocks_out && n_pairs && blocks_per_pair) memset(blocks_out, 0, n_pairs * blocks_per_pair * sizeof *blocks_out);
    return no_throw(c, [&]() -> int {
        c->file_errors.assign(n, std::string());
        c->pair_errors.assign(n_pairs, std::string());
        int rc = rg_bind_device(c);
        if (rc != RG_OK || !n || !n_pairs) return rc;
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        if (groups.size() != 1)
            return rg_set_err(c, RG_ERR_REFUSED, "No comparison: the %zu files would be decoded in %zu groups, and the copies of a pair must lie on the device together", n,
                              groups.size());
        return compare_group(c, paths, n, pairs, n_pairs, o, out, blocks_out, blocks_per_pair, lag_sums);
    });
}

extern "C" const char *rg_compare_error(const rg_ctx *c, size_t pair) { return c && pair < c->pair_errors.size() ? c->pair_errors[pair].c_str() : ""; }

// ---- rg_same_recording_xrate: per group the resampler (rg_resample.hip) and the fingerprint kernels on its output, the match once
// (include/mp3rgain_amd_resample.h).  The codes are kept as rg_same_recording keeps them; a group's resampled signals lie in
// c->d_rs_y while its tiles run.
static int xrate_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, FpCall *call, rg_xrate_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    std::vector<PcmRec> recs;  // plane: the track's place in `tracks`
    std::vector<RgRsTrack> tracks(n + 1);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_rs_track(i, g.descs[k], g.arena_bytes, &tracks[recs.size()], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, recs.size()});
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        std::vector<RgFpTrack> fp(recs.size() + 1);
        uint64_t codes = 0;
        for (size_t t = 0; t < recs.size(); ++t) {
            rg_xr_fp_track(tracks[t], 0, &fp[t]);
            codes += fp[t].frames ? fp[t].frames - 1u : 0u;
        }
        int rc = fp_codes_grow(c, call->used, call->used + (size_t)codes + 4, c->file_stream());
        if (rc != RG_OK) return rc;
        std::vector<uint32_t> nonfinite(recs.size());
        rc = rg_xrate_device(c, c->d_arena.p, tracks.data(), fp.data(), recs.size(), call->used, c->d_fp_codes.p, nullptr, nonfinite.data(), c->file_stream());
        if (rc != RG_OK) return rc;
        call->used += (size_t)codes;
        for (const PcmRec &r : recs)
            rg_xr_fill(g.descs[r.k], tracks[r.plane], fp[r.plane], dropped_frames(g, r.k), nonfinite[r.plane], (uint32_t)(first + g.slot[r.k]), 0,
                       &out[g.slot[r.k]]);
        return RG_OK;
    };
    return pcm_scan_group(g, "fingerprint", RG_RS_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_same_recording_xrate(rg_ctx *c, const char *const *paths, size_t n, const rg_fingerprint_opts *opts, rg_xrate_result *out,
                                       rg_fingerprint_pair *pairs, size_t max_pairs, size_t *n_pairs, uint32_t *codes_out, size_t codes_cap) {
    if (!c || !n_pairs || (max_pairs && !pairs) || (codes_cap && !codes_out)) return RG_ERR_INVALID_ARG;
    *n_pairs = 0;
    if (n > 65535) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_same_recording_xrate: %zu files, at most 65535 in one call", n);
    FpCall call;
    rg_fingerprint_opts o;
    int rc = pcm_scan_call(c, paths, n, opts, out, rg_xr_options,
                           [&](size_t first, size_t cnt, const rg_fingerprint_opts &) { return xrate_group(c, paths, first, cnt, &call, out); });
    if (rc != RG_OK || n == 0) return rc;
    char err[256] = "";
    (void)rg_xr_options(opts, &o, err, sizeof err);  // (the call above has checked them)
    return no_throw(c, [&]() -> int {
        std::vector<uint32_t> counts(n), rates(n);
        std::vector<uint64_t> at(n);
        for (size_t i = 0; i < n; ++i) {  // a failing file has no codes and takes part in no pair; every other is at 11025 Hz now
            const bool ok = out[i].status == RG_OK;
            counts[i] = ok ? out[i].codes : 0u;
            rates[i] = ok && !(out[i].flags & RG_FP_RATE) ? RG_RS_RATE_OUT : 0u;
            at[i] = ok ? out[i].codes_at : 0u;
        }
        std::vector<uint32_t> groups, matches;
        const int mrc = fp_match_call(c, n, counts, rates, at, o, call.used, pairs, max_pairs, n_pairs, codes_out, codes_cap, &groups, &matches);
        if (mrc != RG_OK) return mrc;
        for (size_t i = 0; i < n; ++i) {
            if (out[i].status != RG_OK) continue;
            out[i].group = groups[i];
            out[i].matches = matches[i];
            if (!codes_out || out[i].codes_at + out[i].codes > codes_cap) out[i].codes_at = UINT64_MAX;
        }
        return RG_OK;
    });
}

// ---- rg_tempo: the onset kernels of rg_tempo.hip per group, and the window and finish kernels behind them ------------------
// A group's onset curves lie in c->d_tp_onsets while its stage 2 runs; the caller's copy of them is filled group by group.
namespace {
struct TempoCall {
    uint16_t *onsets_out;
    size_t cap, used = 0;  // onsets the caller's array holds, and those already in it
};
}  // namespace

static int tempo_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_tempo_opts &o, TempoCall *call, rg_tempo_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    std::vector<PcmRec> recs;  // plane: the track's place in `tracks`
    std::vector<RgFpTrack> tracks(n + 1);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_tp_track(i, g.descs[k], g.arena_bytes, &tracks[recs.size()], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, recs.size()});
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        hipStream_t s = c->file_stream();
        uint64_t fmt_tile[4], onsets = 0;
        (void)rg_fp_plan(tracks.data(), recs.size(), fmt_tile, 0, 0);
        for (size_t t = 0; t < recs.size(); ++t) onsets += tracks[t].frames ? tracks[t].frames - 1u : 0u;
        RG_HIP(c, c->d_tp_onsets.reserve((size_t)onsets + 8));
        std::vector<uint32_t> nonfinite(recs.size());
        int rc = rg_tempo_onsets_device(c, c->d_arena.p, tracks.data(), recs.size(), c->d_tp_onsets.p, nullptr, nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        std::vector<RgTpTrack> s2(recs.size());
        std::vector<RgTpFinish> fin(recs.size());
        for (const PcmRec &r : recs) {
            rg_tp_stage2_track(g.descs[r.k].sample_rate, tracks[r.plane].frames ? tracks[r.plane].frames - 1u : 0u, o, &s2[r.plane]);
            s2[r.plane].onsets_at = tracks[r.plane].codes_at;
        }
        rc = rg_tempo_stage2_device(c, c->d_tp_onsets.p, s2.data(), recs.size(), o, fin.data(), nullptr, s);
        if (rc != RG_OK) return rc;
        // the caller's copy: whole tracks, as many as fit
        size_t fit = 0;
        for (const PcmRec &r : recs) {
            const RgFpTrack &t = tracks[r.plane];
            const uint64_t k = t.frames ? t.frames - 1u : 0u;
            uint64_t at = UINT64_MAX;
            if (call->onsets_out && fit == t.codes_at && call->used + t.codes_at + k <= call->cap) {
                at = call->used + t.codes_at;
                fit = (size_t)(t.codes_at + k);
            }
            rg_tp_fill(&g.descs[r.k], g.descs[r.k].sample_rate, t.frames, s2[r.plane], fin[r.plane], dropped_frames(g, r.k), nonfinite[r.plane], at,
                       &out[g.slot[r.k]]);
            out[g.slot[r.k]].band_frames = 0;  // the file call gives no band energies
        }
        if (fit) {
            RG_HIP(c, hipMemcpyAsync(call->onsets_out + call->used, c->d_tp_onsets.p, fit * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
            RG_HIP(c, hipStreamSynchronize(s));
            call->used += fit;
        }
        return RG_OK;
    };
    return pcm_scan_group(g, "tempo", RG_TEMPO_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_tempo(rg_ctx *c, const char *const *paths, size_t n, const rg_tempo_opts *opts, rg_tempo_result *out, uint16_t *onsets_out,
                        size_t onsets_cap) {
    if (!c || (onsets_cap && !onsets_out)) return RG_ERR_INVALID_ARG;
    TempoCall call{onsets_out, onsets_out ? onsets_cap : 0};
    return pcm_scan_call(c, paths, n, opts, out, rg_tp_options,
                         [&](size_t first, size_t cnt, const rg_tempo_opts &o) { return tempo_group(c, paths, first, cnt, o, &call, out); });
}

// ---- rg_key: the decimation, tiles and finish kernels of rg_key.hip per group ----------------------------------------------
// A group's decimated signals and chroma rows lie in c->d_key_decim and c->d_key_rows; the caller's copy of the rows is filled
// group by group.
namespace {
struct KeyCall {
    uint16_t *chroma_out;
    size_t cap, used = 0;  // rows the caller's array holds, and those already in it
};
}  // namespace

static int key_group(rg_ctx *c, const char *const *paths, size_t first, size_t n, const rg_key_opts &o, KeyCall *call, rg_key_result *out) {
    FileGroup g(c, paths, first, n);
    out += first;
    std::vector<PcmRec> recs;  // plane: the track's place in `tracks`
    std::vector<RgKeyTrack> tracks(n + 1);
    const auto add = [&](size_t k, size_t i, char *err) -> int {
        const int rc = rg_key_track(i, g.descs[k], g.arena_bytes, &tracks[recs.size()], err, kPcmErrLen);
        if (rc != RG_OK) return rc;
        recs.push_back(PcmRec{k, recs.size()});
        return RG_OK;
    };
    const auto finish = [&]() -> int {
        if (recs.empty()) return RG_OK;
        hipStream_t s = c->file_stream();
        std::vector<uint32_t> nonfinite(recs.size());
        std::vector<RgKeyFinish> fin(recs.size());
        const int rc = rg_key_device(c, c->d_arena.p, tracks.data(), recs.size(), o, false, fin.data(), nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        // the caller's copy: whole tracks, as many as fit
        size_t fit = 0;
        for (const PcmRec &r : recs) {
            const RgKeyTrack &t = tracks[r.plane];
            uint64_t at = UINT64_MAX;
            if (call->chroma_out && fit == t.rows_at && call->used + t.rows_at + t.rows <= call->cap) {
                at = call->used + t.rows_at;
                fit = (size_t)(t.rows_at + t.rows);
            }
            rg_key_fill(&g.descs[r.k], &t, t.rows, fin[r.plane], dropped_frames(g, r.k), nonfinite[r.plane], at, &out[g.slot[r.k]]);
        }
        if (fit) {
            RG_HIP(c, hipMemcpyAsync(call->chroma_out + call->used * RG_KEY_CHROMA, c->d_key_rows.p, fit * RG_KEY_CHROMA * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
            RG_HIP(c, hipStreamSynchronize(s));
            call->used += fit;
        }
        return RG_OK;
    };
    return pcm_scan_group(g, "key", RG_KEY_MAX_CHANNELS, out, add, finish);
}

extern "C" int rg_key(rg_ctx *c, const char *const *paths, size_t n, const rg_key_opts *opts, rg_key_result *out, uint16_t *chroma_out, size_t chroma_cap) {
    if (!c || (chroma_cap && !chroma_out)) return RG_ERR_INVALID_ARG;
    KeyCall call{chroma_out, chroma_out ? chroma_cap : 0};
    return pcm_scan_call(c, paths, n, opts, out, rg_key_options,
                         [&](size_t first, size_t cnt, const rg_key_opts &o) { return key_group(c, paths, first, cnt, o, &call, out); });
}
