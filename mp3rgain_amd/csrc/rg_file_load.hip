// rg_file_load.hip -- one file of the file layer into a LoadedAudio, by content: RIFF/WAVE bytes, a native FLAC stream, an
// MPEG Layer III stream (bare, or the selected track of an MP4 file) by one of the three host routes, anything else through
// the decoder command; what a loaded file comes to before any analysis (file_outcome); and the files of a call on the
// host's cores (load_many).  No device work except what load_many hands to the loader pipeline (rg_mp3_pipe.hip).
#include <errno.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <new>
#include <stdexcept>
#include <thread>

#include "../../include/mp3rgain_amd_demux.h"
#include "../../include/mp3rgain_amd_mp4.h"
#include "rg_files.h"
#include "rg_r128.h"

namespace rgf {

std::vector<LoadedAudio> &file_pool(rg_ctx *c, size_t n) {
    if (!c->file_pool) {
        c->file_pool = new std::vector<LoadedAudio>();
        c->file_pool_free = [](void *p) { delete static_cast<std::vector<LoadedAudio> *>(p); };
    }
    std::vector<LoadedAudio> &pool = *static_cast<std::vector<LoadedAudio> *>(c->file_pool);
    if (pool.size() < n) pool.resize(n);
    for (size_t i = 0; i < n; ++i) pool[i].reset();
    return pool;
}

int load_flac(int route, const char *path, LoadedAudio *out, std::string *err) {
    rg_flac_info si;
    const int rc = rg_flac_index_vec(out->file_bytes.data(), out->file_bytes.size(), &out->flac_frames, &si);
    if (rc == RG_FLAC_ERR_UNSUPPORTED) {
        *err = std::string("Failed to create decoder: ") + path + " (FLAC of " + std::to_string(si.bits_per_sample) +
               " bits per sample; this library decodes 4-24: set a decoder command, rg_set_decoder_command)";
        return kFlacNotHere;
    }
    if (rc != RG_FLAC_OK) {
        *err = std::string("Failed to probe format: ") + path + " (" + rg_flac_last_error() + ")";
        return RG_ERR_FORMAT;
    }
    out->kind = LoadedAudio::Flac;
    out->sample_rate = si.sample_rate;
    out->channels = si.channels;
    out->flac_bps = si.bits_per_sample;
    out->frames = si.frames;
    if (route != 0) return RG_OK;
    // the host decoder
    std::vector<int32_t> pcm((size_t)si.frames * si.channels + 1);
    int32_t *planes[8];
    for (uint32_t ch = 0; ch < si.channels; ++ch) planes[ch] = pcm.data() + (size_t)ch * si.frames;
    rg_flac_info di;
    if (rg_flac_decode_vec(out->file_bytes.data(), out->file_bytes.size(), out->flac_frames, si, planes, si.frames, &di, nullptr) != RG_FLAC_OK) {
        *err = std::string("Failed to decode: ") + path;
        return RG_ERR_FORMAT;
    }
    const uint32_t eb = flac_elem_bytes(si.bits_per_sample), sh = flac_shift(si.bits_per_sample);
    out->frames = di.frames;
    out->flac_decoded = di.audio_frames;
    out->flac_dropped = di.dropped_frames;
    out->flac_pcm.resize((size_t)di.frames * si.channels * eb);
    for (uint32_t ch = 0; ch < si.channels; ++ch) {
        const int32_t *src = planes[ch];
        if (eb == 2) {
            int16_t *dst = reinterpret_cast<int16_t *>(out->flac_pcm.data()) + (size_t)ch * di.frames;
            for (uint64_t i = 0; i < di.frames; ++i) dst[i] = (int16_t)((uint32_t)src[i] << sh);
        } else {
            int32_t *dst = reinterpret_cast<int32_t *>(out->flac_pcm.data()) + (size_t)ch * di.frames;
            for (uint64_t i = 0; i < di.frames; ++i) dst[i] = (int32_t)((uint32_t)src[i] << sh);
        }
    }
    out->flac_frames.clear();
    return RG_OK;
}

// Host threads this process may really run: the affinity mask, cut by the cgroup CPU quota if there is one (a container
// with 16 CPUs' worth of quota on a 256-core host sees all 256 in its mask; 256 loader threads then only fight).
unsigned usable_cores() {
    unsigned n = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = (unsigned)CPU_COUNT(&set);
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
        char q[64];
        double period = 0.0;
        if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0.0) {
            const double cpus = atof(q) / period;
            if (cpus >= 1.0 && cpus < (double)n) n = (unsigned)(cpus + 0.5);
        }
        fclose(f);
    } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
        double quota = -1.0, period = 0.0;
        if (fscanf(g, "%lf", &quota) != 1) quota = -1.0;
        fclose(g);
        if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(h, "%lf", &period) != 1) period = 0.0;
            fclose(h);
        }
        if (quota > 0.0 && period > 0.0 && quota / period >= 1.0 && quota / period < (double)n) n = (unsigned)(quota / period + 0.5);
    }
    return n < 1 ? 1 : n;
}

namespace {

// FLAC in an Ogg container ("OggS" page whose first packet starts 0x7F "FLAC"): not decoded here
bool is_ogg_flac(const uint8_t *d, size_t len) {
    if (len < 27 || memcmp(d, "OggS", 4) != 0) return false;
    const size_t body = 27 + (size_t)d[26];
    return len >= body + 5 && d[body] == 0x7F && memcmp(d + body + 1, "FLAC", 4) == 0;
}

bool read_all(FILE *f, std::vector<uint8_t> *out) {
    uint8_t chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) out->insert(out->end(), chunk, chunk + n);
    return !ferror(f);
}

std::string shell_quote(const char *s) {
    std::string q = "'";
    for (; *s; ++s) {
        if (*s == '\'') q += "'\\''";
        else q += *s;
    }
    return q + "'";
}

// The three host routes of an MPEG Layer III stream (`si`: what rg_mp3_scan found): tuning key 6 = 2, 1, 0.  The decoder's status.
int decode_mpeg_host(int gpu_decode, const std::vector<uint8_t> &bytes, const rg_mp3_stream_info &si, LoadedAudio *out) {
    rg_mp3_stream_info di;
    int rc;
    if (gpu_decode == 2) {  // only the frame walk here: side information and where each granule's bits are
        rc = rg_mp3_index_stream(bytes.data(), bytes.size(), &out->main_stream, &out->recs, &di);
        out->n_units = out->recs.size();
    } else if (gpu_decode) {  // stage A here (frame walk, side info, reservoir, scalefactors, Huffman), the rest on the device
        const uint64_t cap = (uint64_t)si.audio_frames * (si.mpeg_version == 1 ? 2u : 1u) * si.channels;
        out->is.assign((size_t)cap * 576, 0);
        out->units.assign((size_t)cap, rg_mp3_unit{});
        rc = rg_mp3_parse_units(bytes.data(), bytes.size(), out->is.data(), out->units.data(), cap, &out->n_units, &di);
    } else {
        out->planar.assign((size_t)si.frames * si.channels, 0.0f);
        rc = rg_mp3_decode_f32(bytes.data(), bytes.size(), out->planar.data(), si.channels == 2 ? out->planar.data() + si.frames : nullptr,
                               si.frames, &di);
        if (rc == RG_MP3DEC_OK && si.channels == 2 && di.frames != si.frames)  // dropped frames shortened the track: close the gap between the planes
            memmove(out->planar.data() + di.frames, out->planar.data() + si.frames, sizeof(float) * (size_t)di.frames);
    }
    if (rc != RG_MP3DEC_OK) return rc;
    out->sample_rate = di.sample_rate;
    out->channels = di.channels;
    out->frames = di.frames;
    out->mp3_skipped = di.skipped_frames;
    if (gpu_decode) out->lsf = di.mpeg_version == 1 ? 0u : 1u;
    out->kind = gpu_decode ? LoadedAudio::Split : LoadedAudio::Planar;
    return rc;
}

// The decoder command's stdout (a WAV stream) into out->wav.  "{}" = the path, quoted (appended when the template has none).
int run_decoder_command(std::string cmd, int mp4_track, const char *path, LoadedAudio *out, std::string *err) {
    {   // "{track}" = index of the selected audio track (ffmpeg: -map 0:a:{track})
        const std::string tn = std::to_string(mp4_track);
        for (size_t at = cmd.find("{track}"); at != std::string::npos; at = cmd.find("{track}", at + tn.size())) cmd.replace(at, 7, tn);
    }
    const std::string q = shell_quote(path);
    size_t at = cmd.find("{}");
    if (at == std::string::npos) cmd += " " + q;
    else
        for (; at != std::string::npos; at = cmd.find("{}", at + q.size())) cmd.replace(at, 2, q);
    FILE *p = popen(cmd.c_str(), "r");
    if (!p) {
        *err = std::string("Failed to run decoder: ") + strerror(errno);
        return RG_ERR_IO;
    }
    out->wav.clear();
    const bool rd = read_all(p, &out->wav);
    const int status = pclose(p);
    if (!rd || status != 0 || out->wav.empty()) {
        *err = std::string("Failed to probe format: ") + path + " (decoder command exited with status " + std::to_string(status) + ")";
        return RG_ERR_FORMAT;
    }
    return RG_OK;
}

int load_audio_for_impl(const std::string &decoder_cmd, int gpu_decode, const char *path, LoadedAudio *out, std::string *err, int32_t track_index,
                        int flac_route) {
    char msg[1024];
    auto fail = [&](int code, const char *fmt, const char *a, int b = 0) {
        snprintf(msg, sizeof msg, fmt, a, b);
        *err = msg;
        return code;
    };
    if (!path) return fail(RG_ERR_INVALID_ARG, "null path%s", "");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RG_ERR_IO, "Failed to open: %s", path);  // src/replaygain.rs:804-805
    std::vector<uint8_t> &bytes = out->file_bytes;
    bytes.clear();
    const bool ok = read_all(f, &bytes);
    fclose(f);
    if (!ok) return fail(RG_ERR_IO, "Failed to read: %s", path);
    if (bytes.size() >= 12 && memcmp(bytes.data(), "RIFF", 4) == 0 && memcmp(bytes.data() + 8, "WAVE", 4) == 0) {
        out->wav.swap(bytes);
        return RG_OK;
    }
    // FLAC before the MPEG probe: a FLAC payload can hold byte runs the Layer III scanner would take for frames
    bool to_command = false;
    if (rg_flac_is_flac(bytes.data(), bytes.size())) {
        const int rc = load_flac(flac_route, path, out, err);
        if (rc != kFlacNotHere) return rc;
        out->kind = LoadedAudio::Wav;
        if (decoder_cmd.empty()) return RG_ERR_FORMAT;
        to_command = true;
    } else if (is_ogg_flac(bytes.data(), bytes.size())) {
        if (decoder_cmd.empty())
            return fail(RG_ERR_FORMAT, "Failed to create decoder: %s (FLAC in Ogg is not decoded by this library: set a decoder command, rg_set_decoder_command)", path);
        to_command = true;
    }
    const bool mp4 = !to_command && bytes.size() >= 8 && memcmp(bytes.data() + 4, "ftyp", 4) == 0;
    out->is_mp4 = rg_mp4_is_mp4_data(bytes.data(), bytes.size()) != 0;  // detect_file_type, src/replaygain.rs:777-783
    int mp4_track = 0;
    bool mp4_mpeg_audio = false;  // the selected track of an MP4 file is MPEG audio: `bytes` now holds its elementary stream
    if (mp4) {
        // ---- ISO base media: the audio tracks the reference would see (src/replaygain.rs:827-836), the one it would pick
        // (:838-851), its rate (:854-857).  MPEG Layer III in MP4 is decoded here, from the sample table; AAC needs the
        // decoder command.
        rg_mp4_audio_track tr[32];
        size_t n_audio = 0;
        bool walked = rg_mp4_audio_tracks(bytes.data(), bytes.size(), tr, 32, &n_audio) == RG_DEMUX_OK;
        // A file this walker cannot read (no moov box), or in which it finds no track of a codec the reference's build
        // decodes, is still the decoder command's to try when there is one: the command is the user's decoder (ALAC in
        // M4A, say), and the authority on what it can read.
        if (!walked && decoder_cmd.empty()) return fail(RG_ERR_FORMAT, "Failed to probe format: %s", path);
        if (walked && n_audio == 0) {
            if (decoder_cmd.empty()) return fail(RG_ERR_FORMAT, "No audio track found%s", "");
            walked = false;
        }
        if (walked) {
            out->n_audio_tracks = (uint32_t)n_audio;
            if (track_index >= 0 && (size_t)track_index >= n_audio) {
                snprintf(msg, sizeof msg, "Track index %d out of range (file has %zu audio track(s))", track_index, n_audio);
                *err = msg;
                return RG_ERR_INVALID_ARG;
            }
            mp4_track = track_index < 0 ? 0 : track_index;
            if (mp4_track >= 32) return fail(RG_ERR_INVALID_ARG, "Track index %d: more audio tracks than this library lists%s", "", mp4_track);
            const rg_mp4_audio_track &t = tr[mp4_track];
            if (t.sample_rate == 0) return fail(RG_ERR_FORMAT, "Unknown sample rate%s", "");
            if (t.codec == RG_CODEC_MP3) {
                // the track's samples are MPEG audio frames: laid end to end they are the stream the library's decoder takes
                size_t n_au = 0;
                if (rg_mp4_access_units(bytes.data(), bytes.size(), (size_t)mp4_track, nullptr, nullptr, 0, &n_au) != RG_DEMUX_OK)
                    return fail(RG_ERR_FORMAT, "Failed to probe format: %s", path);
                std::vector<uint64_t> off(n_au);
                std::vector<uint32_t> sz(n_au);
                size_t got = 0;
                (void)rg_mp4_access_units(bytes.data(), bytes.size(), (size_t)mp4_track, off.data(), sz.data(), n_au, &got);
                std::vector<uint8_t> es;
                for (size_t i = 0; i < got && i < n_au; ++i) es.insert(es.end(), bytes.begin() + (ptrdiff_t)off[i], bytes.begin() + (ptrdiff_t)(off[i] + sz[i]));
                bytes.swap(es);
                mp4_mpeg_audio = true;
                out->mpeg_in_mp4 = true;
            }
        }
    }
    if (!to_command && (!mp4 || mp4_mpeg_audio)) {
        // the probe (src/replaygain.rs:815-822) and the packet loop (:881-904) for an MPEG audio stream
        rg_mp3_stream_info si;
        if (rg_mp3_scan(bytes.data(), bytes.size(), &si) == RG_MP3DEC_OK && si.audio_frames > 0) {
            if (decode_mpeg_host(gpu_decode, bytes, si, out) != RG_MP3DEC_OK) return fail(RG_ERR_FORMAT, "Failed to decode: %s", path);
            return RG_OK;
        }
    }
    if (mp4_mpeg_audio)  // an MPEG audio track whose samples are not Layer III frames this decoder takes (Layer I / II, say)
        return fail(RG_ERR_FORMAT, "Failed to create decoder: %s (the selected track's MPEG audio is not Layer III)", path);
    if (decoder_cmd.empty())  // src/replaygain.rs:861-863 (AAC: the probe succeeded, the codec is missing) / :815-822 (the probe knows no such format)
        return fail(RG_ERR_FORMAT, mp4 ? "Failed to create decoder: %s (an AAC track; no AAC decoder is built into this library: set a decoder command, rg_set_decoder_command)"
                                       : "Failed to probe format: %s (neither MPEG Layer III nor RIFF/WAVE, and no decoder command is set: rg_set_decoder_command)",
                    path);
    return run_decoder_command(decoder_cmd, mp4_track, path, out, err);
}

}  // namespace

// The loaders run on host threads of the library's own: an allocation failure there must come back as a status, not end
// the process in std::terminate.
int load_audio_for(const std::string &decoder_cmd, int gpu_decode, const char *path, LoadedAudio *out, std::string *err, int32_t track_index,
                   int flac_route) {
    try {
        return load_audio_for_impl(decoder_cmd, gpu_decode, path, out, err, track_index, flac_route);
    } catch (const std::bad_alloc &) {
        *err = std::string("Out of memory while loading: ") + (path ? path : "");
        return RG_ERR_NOMEM;
    } catch (const std::exception &ex) {
        *err = std::string("Failed to load: ") + (path ? path : "") + " (" + ex.what() + ")";
        return RG_ERR_FORMAT;
    }
}

int file_outcome(const LoadedAudio &la, int load_rc, const std::string &load_err, const char *path, int32_t track_index, std::string *msg,
                 bool r128) {
    if (load_rc != RG_OK) {
        *msg = load_err;
        return load_rc;
    }
    if (track_index >= 0 && (uint32_t)track_index >= la.n_audio_tracks) {
        char m[128];
        snprintf(m, sizeof m, "Track index %d out of range (file has %u audio track(s))", track_index, la.n_audio_tracks);
        *msg = m;
        return RG_ERR_INVALID_ARG;
    }
    uint32_t rate = la.sample_rate;
    if (la.kind == LoadedAudio::Wav) {
        rg_wav_info wi;
        rate = rg_wav_parse(la.wav.data(), la.wav.size(), &wi) == RG_OK ? wi.sample_rate : 0;
        if (rate == 0) {
            *msg = std::string("Failed to probe format: ") + path;
            return RG_ERR_FORMAT;
        }
    }
    if (r128) {
        if (rg_r128_supported_rate(rate)) return RG_OK;
        char m[128];
        snprintf(m, sizeof m, "Unsupported sample rate: %u Hz. Supported rates: %u to %u", rate, RG_R128_MIN_RATE, RG_R128_MAX_RATE);
        *msg = m;
        return RG_ERR_UNSUPPORTED_RATE;
    }
    if (!rg_supported_rate(rate)) {
        char m[256];
        snprintf(m, sizeof m, "Unsupported sample rate: %u Hz. Supported rates: 96000, 88200, 64000, 48000, 44100, 32000, 24000, "
                              "22050, 16000, 12000, 11025, 8000", rate);
        *msg = m;
        return RG_ERR_UNSUPPORTED_RATE;
    }
    return RG_OK;
}

// Whether stage_loaded can lay out a file that file_outcome passed: a RIFF/WAVE stream of a sample format the de-interleave
// does not read (64-bit float, A-law, mu-law, ...) parses, but fails the whole batch there ("input k: unsupported WAV sample
// format"); rg_analyze_album reports such a file as "Failed to probe format: <path>".
bool stageable(const LoadedAudio &la) {
    if (la.kind != LoadedAudio::Wav) return true;
    rg_wav_info wi;
    return rg_wav_parse(la.wav.data(), la.wav.size(), &wi) == RG_OK && wav_kind(wi) >= 0;
}

// The files of an album, decoded on the host's cores (decode is by far the longest stage of a real run: one core turns
// about 200 s of stereo audio into PCM per second, the GPU analyses 8 million).  Errors keep the reference's order: the
// first failing file in input order is the one reported (src/replaygain.rs:1055).
int load_many(rg_ctx *c, const char *const *paths, size_t n, std::vector<LoadedAudio> *out, const LoadOpts &opts, std::vector<int> *rcs_out,
              std::vector<std::string> *errs_out, PartsRun *parts) {
    std::vector<int> rcs(n, RG_OK);
    std::vector<std::string> errs(n);
    if (c->gpu_mp3_decode >= 3 && n) {
        const int prc = pipe_load_many(c, paths, n, out, &rcs, &errs, opts, parts);
        if (prc != RG_OK) return prc;
    } else {
        unsigned workers = c->loader_threads ? c->loader_threads : usable_cores();
        if (workers > n) workers = (unsigned)n;
        std::atomic<size_t> next{0};
        const std::string cmd = opts.decoder_command ? c->decoder_cmd : std::string();
        const int32_t track_index = opts.track_index;
        const int gpu_decode = c->gpu_mp3_decode;
        const int flac_route = c->gpu_flac_decode;
        auto work = [&]() {
            for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1))
                rcs[i] = load_audio_for(cmd, gpu_decode, paths[i], &(*out)[i], &errs[i], track_index, flac_route);  // (*out) holds >= n entries
        };
        if (workers <= 1) {
            work();
        } else {
            std::vector<std::thread> pool;
            for (unsigned w = 0; w < workers; ++w) pool.emplace_back(work);
            for (auto &t : pool) t.join();
        }
    }
    if (rcs_out) {  // per-file outcome wanted: nothing aborts
        rcs_out->swap(rcs);
        errs_out->swap(errs);
        return RG_OK;
    }
    for (size_t i = 0; i < n; ++i)
        if (rcs[i] != RG_OK) return rg_set_err(c, rcs[i], "%s", errs[i].c_str());
    return RG_OK;
}

}  // namespace rgf

unsigned rg_usable_cores() { return rgf::usable_cores(); }
