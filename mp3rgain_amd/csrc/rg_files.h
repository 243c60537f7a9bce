// rg_files.h -- internal: what the translation units of the file layer share.  rg_wav.hip (RIFF/WAVE, de-interleave),
// rg_file_load.hip (per-file loaders), rg_file_stage.hip (loaded files -> arena), rg_mp3_pipe.hip (the MP3 loader pipeline),
// rg_files.hip (the ReplayGain and R 128 entry points), rg_file_verify.hip (the verify and rip entry points),
// rg_file_hooks.hip (measurement and parity hooks).  Nothing outside them includes it.
#pragma once

#include <string.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mp3rgain_amd.h"
#include "../../include/mp3rgain_amd_dec.h"
#include "rg_ctx.h"
#include "rg_flac.h"
#include "rg_mp3_frame.h"
#include "rg_mp3dev.h"
#include "rg_mp3dev_host.h"

namespace rgf {

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// ---- rg_wav.hip ---------------------------------------------------------------------------------------------------------
struct WavItem {
    const uint8_t *bytes;
    rg_wav_info info;
    int kind;
    uint64_t src_off;  // in the interleaved staging buffer
    uint64_t src_len;
};
int wav_kind(const rg_wav_info &w);  // WavKind, or -1: a sample format the de-interleave does not read
// dwChannelMask of a RIFF/WAVE stream whose format tag is WAVE_FORMAT_EXTENSIBLE (0xFFFE); 0 for any other stream
uint32_t wav_channel_mask(const void *data, size_t len);
// Input `i` of a batch, a RIFF/WAVE stream: `it`, and `d` at the arena's *dst_total; both totals move past it.  An error is
// "input <i> ..." (rg_analyze_album_begin reads the index back).
int wav_layout(rg_ctx *c, size_t i, const void *bytes, size_t len, WavItem *it, rg_track_desc *d, size_t *src_total, size_t *dst_total);
// its interleaved samples to c->d_wav and from there, planar, to `dst`, on stream `fs`
int wav_copy_launch(rg_ctx *c, const WavItem &it, unsigned char *dst, hipStream_t fs);
// parse, copy to HBM, de-interleave: on return `descs` describe the planar arena c->d_arena
int stage_wavs(rg_ctx *c, const void *const *wav, const size_t *wav_len, size_t n, std::vector<rg_track_desc> *descs, size_t *arena_bytes);

// ---- rg_file_load.hip ---------------------------------------------------------------------------------------------------
// One input of the file layer after loading: either the bytes of a WAV stream, or planar f32 PCM from the MP3 decoder
struct LoadedAudio {
    enum Kind {
        Wav,     // `wav`: a RIFF/WAVE stream (a file, or the decoder command's stdout); also "nothing yet"
        Planar,  // `planar` is valid: the host MP3 decoder's PCM
        Split,   // split decode (tuning key 6 = 1, 2): see `is` and `main_stream`
        Staged,  // tuning key 6 = 3: the loader pipeline has decoded the stream into the arena already
        Flac     // a native FLAC stream: see `flac_frames`
    };
    Kind kind = Wav;
    std::vector<uint8_t> wav;
    std::vector<float> planar;  // [channels][frames]
    uint32_t sample_rate = 0, channels = 0;
    uint64_t frames = 0;
    // split decode (tuning key 6): stage A ran on the host, stages B-E will run on the device into the arena
    std::vector<int16_t> is;
    std::vector<rg_mp3_unit> units;
    uint64_t n_units = 0;
    uint32_t lsf = 0;
    // tuning key 6 = 2: the host only walks the frames; scalefactors and Huffman run on the device as well
    std::vector<uint8_t> main_stream;
    std::vector<RgMp3HuffRec> recs;
    std::vector<uint8_t> file_bytes;  // the file as read
    bool is_mp4 = false;
    uint32_t n_audio_tracks = 1;  // an MP4 file: what its sample tables say (include/mp3rgain_amd_demux.h); anything else has one
    // Staged: planar f32 at arena_off; `frames` is what the device found decodable
    uint64_t arena_off = 0;
    uint64_t walked_frames = 0;  // PCM frames if every walked frame decodes: what the arena is laid out for
    uint32_t result_index = 0;
    // Flac (file_bytes): its frame index for the device route (tuning key 14 = 1), or the host decoder's PCM
    // already in the arena's format (key 14 = 0); `frames` is then the decoded length, else what the index walked
    std::vector<rg_flac_frame> flac_frames;
    std::vector<uint8_t> flac_pcm;
    uint32_t flac_bps = 0;
    uint32_t flac_decoded = 0, flac_dropped = 0;  // key 14 = 0: FLAC frames the host decoder decoded / dropped
    uint32_t mp3_skipped = 0;    // Planar / Split: frames the host's decoder or frame walk dropped (rg_mp3_stream_info::skipped_frames)
    bool mpeg_in_mp4 = false;    // the MPEG stream is the selected track of an MP4 file, not the file itself
    // ready for the next file; the vectors keep their capacity
    void reset() {
        wav.clear(); planar.clear(); is.clear(); units.clear(); main_stream.clear(); recs.clear(); file_bytes.clear();
        flac_frames.clear(); flac_pcm.clear(); flac_bps = 0; flac_decoded = flac_dropped = 0;
        sample_rate = channels = 0; frames = 0; n_units = 0; lsf = 0;
        kind = Wav; is_mp4 = false;
        arena_off = 0; walked_frames = 0; result_index = 0; n_audio_tracks = 1;
        mp3_skipped = 0; mpeg_in_mp4 = false;
    }
};

// the arena format of FLAC PCM (rg_flac.h: flac_elem_bytes, flac_shift) as a track descriptor's
inline uint16_t flac_format(uint32_t bps) { return bps <= 16 ? RG_FMT_S16_PLANAR : RG_FMT_S32_PLANAR; }

constexpr int kFlacNotHere = 1;  // load_flac: a FLAC stream this library does not decode (the decoder command's to try)

struct PartsRun;
// What a call asks of the loaders, handed down to every loader thread: nothing of it lives in the context.
struct LoadOpts {
    int32_t track_index = -1;      // Some(idx) among the audio tracks of a container (src/replaygain.rs:838-851); -1 = None
    bool decoder_command = true;   // false: the loaders see no decoder command, whatever rg_set_decoder_command has set
    bool keep_mpeg_bytes = false;  // the loader pipeline keeps an MPEG stream's bytes as read (rg_mp3_verify: its compaction works in place)
};
// the context's pool of LoadedAudio (rg_ctx::file_pool): entry i serves the i-th file of a call
std::vector<LoadedAudio> &file_pool(rg_ctx *c, size_t n);
// A native FLAC stream in `out->file_bytes`: the frame walk, and with route 0 the host decoder's PCM in the arena's format.
int load_flac(int route, const char *path, LoadedAudio *out, std::string *err);
// Load one file (no device work; safe to call from several threads at once as long as `err` is per call).
// RIFF/WAVE: the bytes; MPEG Layer III: decoded planar f32; anything else: the decoder command's stdout.
// A native FLAC stream (also behind an ID3v2 tag): its frame index, or PCM from the host decoder (flac_route = tuning key 14).
int load_audio_for(const std::string &decoder_cmd, int gpu_decode, const char *path, LoadedAudio *out, std::string *err, int32_t track_index,
                   int flac_route);
unsigned usable_cores();
// What one file of a list comes to before any analysis, in the order the reference meets its errors
// (src/replaygain.rs:804-873): open / read, track selection, probe, sample rate.  RG_OK, or the code with `msg` set.
int file_outcome(const LoadedAudio &la, int load_rc, const std::string &load_err, const char *path, int32_t track_index, std::string *msg,
                 bool r128 = false /* the EBU R 128 path's rate rule */);
bool stageable(const LoadedAudio &la);
// entry i of `out` <- file i; with rcs_out / errs_out the per-file outcome is wanted and nothing aborts
int load_many(rg_ctx *c, const char *const *paths, size_t n, std::vector<LoadedAudio> *out, const LoadOpts &opts,
              std::vector<int> *rcs_out = nullptr, std::vector<std::string> *errs_out = nullptr, PartsRun *parts = nullptr);
// `out` is entry 0 of the context's pool
inline int load_one(rg_ctx *c, const char *path, std::vector<LoadedAudio> *pool, const LoadOpts &opts) { return load_many(c, &path, 1, pool, opts); }

// ---- rg_file_stage.hip --------------------------------------------------------------------------------------------------
int arena_reserve_keep(rg_ctx *c, size_t need, size_t keep);
// FLAC frames of one input that decoded / were dropped (zero for an input that is not a FLAC stream)
struct FlacCounts {
    uint32_t decoded, dropped;
};
// `flac_counts`: null, or entry i <- the counts of input i (the parity hook rg_flac_stage_device_batch reports them)
int stage_loaded(rg_ctx *c, const std::vector<LoadedAudio> &in, size_t n, std::vector<rg_track_desc> *descs, size_t *arena_bytes,
                 std::vector<FlacCounts> *flac_counts = nullptr);

// ---- rg_mp3_pipe.hip ----------------------------------------------------------------------------------------------------
// The loader pipeline of tuning key 6 = 3 (the default).
//
// Host threads do the least an MPEG stream allows: read the file, walk its frame headers, and strip headers and side
// information from the main data (rg_mp3_compact_stream).  Each stream's main data and slots go into a pinned staging
// block; a block that is full (or holds enough granules to fill the GPU) is a chunk, and the calling thread sends chunks
// to the device as they close: one H2D copy on the copy stream, then the frame parser, Huffman and back-half
// kernels on the file stream, writing PCM straight into the analysis arena.  Three staging blocks and two device copies
// rotate, so reading files, copying chunk k + 1 and decoding chunk k overlap.  How many frames of a stream decode is the
// device's finding (rg_mp3_frames_kernel); the arena is laid out for "all of them" and the counts come back at the end.
struct Mp3Stage {
    uint8_t *p = nullptr;
    size_t cap = 0;
    hipEvent_t staged = nullptr;  // H2D of the block's last chunk
    // room for `need` bytes; the block is idle, what it held is not kept
    hipError_t grow(size_t need) {
        if (cap >= need) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = need + need / 8;
        const hipError_t e = hipHostMalloc((void **)&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
};
struct Mp3Scratch {
    uint8_t *p = nullptr;
    size_t cap = 0;
    std::vector<uint8_t> slots;
    std::vector<uint64_t> tiles;
    // room for a stream of `len` bytes and the 64 zero bytes behind it; what the buffer held is kept
    bool reserve(size_t len) {
        if (cap >= len + 64) return true;
        uint8_t *q = static_cast<uint8_t *>(realloc(p, len + 64));
        if (!q) return false;
        p = q;
        cap = len + 64;
        return true;
    }
};
struct Mp3Pipe {
    static constexpr int NSTAGE = 3;
    Mp3Stage stage[NSTAGE];
    std::vector<Mp3Scratch> scratch;  // one per loader thread
    std::vector<hipEvent_t> part_ev;  // album parts: per chunk [2k] its decode is done, [2k + 1] its frame counts are on the host
    ~Mp3Pipe() {
        for (Mp3Stage &st : stage) {
            if (st.p) (void)hipHostFree(st.p);
            if (st.staged) (void)hipEventDestroy(st.staged);
        }
        for (Mp3Scratch &sc : scratch) free(sc.p);
        for (hipEvent_t e : part_ev) (void)hipEventDestroy(e);
    }
};
Mp3Pipe &mp3_pipe(rg_ctx *c);

// One compacted stream (rg_mp3_compact_stream: main data, slots, tiles) in a pinned staging block, from offset `base` on
struct StreamLayout {
    size_t main_off, slots_off, tiles_off, end;
};
inline StreamLayout stream_layout(size_t base, size_t main_len, size_t slot_bytes, size_t tile_bytes) {
    StreamLayout l;
    l.main_off = base;
    l.slots_off = l.main_off + align64(main_len + 8);
    l.tiles_off = l.slots_off + align64(slot_bytes);
    l.end = l.tiles_off + align64(tile_bytes);
    return l;
}
// (one large copy per stream: it leaves the cache-resident scratch buffer with streaming stores.  Gathering the frames'
// main data straight into the block instead -- a frame list first, no compaction in place -- writes the block in
// pieces of a few hundred bytes, each a read-for-ownership of lines nobody will read here, and was slower from
// 128 kb/s up: commit a661d6a, profiles/r06_host_loader.txt)
inline void copy_stream_into(uint8_t *dst, const StreamLayout &l, const Mp3Scratch &sc, size_t main_len) {
    memcpy(dst + l.main_off, sc.p, main_len);
    memset(dst + l.main_off + main_len, 0, l.slots_off - l.main_off - main_len);  // the bit reader looks a few bytes ahead
    memcpy(dst + l.slots_off, sc.slots.data(), sc.slots.size());
    memcpy(dst + l.tiles_off, sc.tiles.data(), sc.tiles.size() * sizeof(uint64_t));
}
inline RgMp3StreamItem stream_item(const StreamLayout &l, uint32_t n_frames, uint32_t channels, uint32_t sample_rate, uint32_t lsf,
                                   uint32_t result_index, void *d_ch0) {
    RgMp3StreamItem it{};
    it.main_off = l.main_off;
    it.slots_off = l.slots_off;
    it.tiles_off = l.tiles_off;
    it.n_frames = n_frames;
    it.channels = channels;
    it.rate_row = (uint32_t)rg_mp3_rate_row(sample_rate);
    it.lsf = lsf;
    it.result_index = result_index;
    it.d_ch0 = static_cast<float *>(d_ch0);
    return it;
}

// Album parts.  The decode of an album's files is a pipeline of chunks (above); with `PartsRun` the tracks of chunk k are
// analysed -- one enqueue on a pipeline stream that waits for the chunk's decode, album mode -- while chunk k + 1 is copied and
// decoded, instead of all together at the end: where the H2D copy is the longest stage (anything from 128 kb/s up) the analysis
// disappears behind it, and elsewhere it fills the decode kernels' tails.  Each part leaves its [histogram | peak] pack in
// c->d_album_packs and its per-track results in c->h_part_results; u32 adds commute, so the album is the fold of the packs
// (the streamed host ingest and albums larger than the device do the same).  Anything out of the ordinary -- a file that is not
// an MPEG stream or failed, an unsupported rate, a track the fast kernels flag -- drops the parts and the album is analysed the
// plain way from the PCM, which is in the arena either way.
constexpr size_t kMaxParts = 64;
// rg_analyze_albums: the live pack (rg_albums.h) the track of each file of a group is folded into.  The track -> pack maps of
// the group's batches go to pinned memory one after the other (nothing there is rewritten before the group's end, when
// everything has been waited for) and are copied to the device on the batch's stream, in front of the fold.
struct AlbumFold {
    std::vector<int32_t> pack_of;  // per file of the group (the numbering of load_many)
    std::vector<size_t> album_of_pack;  // the albums that have files in the group, in input order: one live pack each
    uint32_t *d_packs = nullptr;   // live pack 0; the carried pack sits one stride in front
    size_t n_packs = 0;
    bool carried = false;          // pack 0 is an album that had files in earlier groups: it starts from the carried pack
    size_t map_used = 0;
};
// the live packs as they were when the group began (zero, or the carried pack): at the group's start, and again when the
// plain route follows parts that were folded already
int fold_init(rg_ctx *c, AlbumFold *f);
// the batch just enqueued (the context's current slot holds its final track histograms and peaks: after the exact repeat),
// `files` its tracks' files in batch order: fold them into their albums' packs on the batch's stream `s`
int fold_batch(rg_ctx *c, AlbumFold *f, const size_t *files, size_t k, hipStream_t s);
struct PartsRun {
    int album = 1;  // 0: track mode (rg_analyze_tracks) -- the same parts without the packs
    AlbumFold *fold = nullptr;  // track mode of rg_analyze_albums: every part is folded into its albums' packs
    bool broken = false;
    size_t n_parts = 0;
    std::vector<size_t> file_of;  // position in c->h_part_results -> file of the call
    std::vector<size_t> pending;  // files of decoded chunks not yet in a part (chunks the device, not the copy, was the longer stage of)
};
// Loads `paths` into `out` (entry i <- file i) with the pipeline: MPEG streams are on their way through the device when
// this returns and their PCM sits in c->d_arena (LoadedAudio::Staged), other inputs are loaded as load_audio_for loads
// them.  rcs / errs: per-file outcome.
int pipe_load_many(rg_ctx *c, const char *const *paths, size_t n, std::vector<LoadedAudio> *out, std::vector<int> *rcs,
                   std::vector<std::string> *errs, const LoadOpts &opts, PartsRun *parts);

// ---- rg_files.hip, rg_file_verify.hip: what every per-file call is made of ----------------------------------------------
// An allocation failure on the host must leave an extern "C" function as a status, not as an exception.
template <typename Fn>
int no_throw(rg_ctx *c, Fn fn) {
    try {
        return fn();
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}
// Files of a long list in groups whose PCM is estimated to stay within a third of the free device memory (rg_files.hip)
void file_groups(rg_ctx *c, const char *const *paths, size_t n, std::vector<std::pair<size_t, size_t>> *groups);
// A per-file call: no messages yet, the device bound, then fn(first, cnt) for each group of the list until one fails the call.
template <typename Fn>
int for_each_group(rg_ctx *c, const char *const *paths, size_t n, Fn fn) {
    return no_throw(c, [&]() -> int {
        c->file_errors.assign(n, std::string());
        int rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        std::vector<std::pair<size_t, size_t>> groups;
        file_groups(c, paths, n, &groups);
        for (const auto &g : groups) {
            rc = fn(g.first, g.second);
            if (rc != RG_OK) return rc;
        }
        return RG_OK;
    });
}

// One group of a call, files [first, first + n) of it, on the route every per-file call takes: load(), then run().  `i` is a
// file's index in the group throughout; the call's numbering, which c->file_errors has, is first + i.
struct FileGroup {
    rg_ctx *const c;
    const char *const *const paths;  // the group's: paths[i]
    const size_t first, n;
    std::vector<LoadedAudio> &in;    // the context's pool: in[i] <- file i
    std::vector<int> rcs;            // load(): per file
    std::vector<std::string> errs;
    // run(): the batch, in[k] being file slot[k] from here on (slot ascends)
    std::vector<size_t> slot;
    std::vector<rg_track_desc> descs;
    std::vector<FlacCounts> counts;  // with want_counts
    size_t arena_bytes = 0;
    bool done = false;               // the batch was staged and `work` has returned RG_OK
    // the route's to set before run()
    bool want_counts = false;        // `counts` is wanted
    bool stop_at_first = false;      // the first failing file in input order fails the call, and so does a failing batch

    FileGroup(rg_ctx *c, const char *const *call_paths, size_t first, size_t n)
        : c(c), paths(call_paths + first), first(first), n(n), in(file_pool(c, n)) {}
    // a status other than RG_OK is the call's, not a file's
    int load(const LoadOpts &opts, PartsRun *parts = nullptr) { return load_many(c, paths, n, &in, opts, &rcs, &errs, parts); }
    // Every file gets its outcome, mark(i, code, text): what loading made of it or, for a file that loaded, screen(i, &text)
    // (*text comes in as the loader's, empty as a rule).  The good files go to the front of the pool (swap keeps every buffer
    // alive for the next call) and into the arena as one batch, which `work()` then has.  A failure of the batch itself -- a
    // WAV of a kind the library cannot stage, a device error -- is every file's of the batch: mark(i, rc, c->err).
    template <typename Screen, typename Mark, typename Work>
    int run(Screen screen, Mark mark, Work work) {
        for (size_t i = 0; i < n; ++i) {
            std::string text = errs[i];
            const int code = rcs[i] != RG_OK ? rcs[i] : screen(i, &text);
            mark(i, code, text);
            if (code != RG_OK && stop_at_first) return rg_set_err(c, code, "%s", text.c_str());
            if (code == RG_OK) slot.push_back(i);
        }
        if (slot.empty()) return RG_OK;
        for (size_t k = 0; k < slot.size(); ++k)
            if (slot[k] != k) std::swap(in[k], in[slot[k]]);
        int rc = stage_loaded(c, in, slot.size(), &descs, &arena_bytes, want_counts ? &counts : nullptr);
        if (rc == RG_OK) rc = work();
        done = rc == RG_OK;
        if (done || stop_at_first) return rc;
        for (size_t i : slot) mark(i, rc, c->err);
        return RG_OK;
    }
    // results in batch order -> the caller's array, by file
    template <typename Result>
    void scatter(const std::vector<Result> &res, Result *out) const {
        for (size_t k = 0; k < slot.size(); ++k) out[slot[k]] = res[k];
    }
};

}  // namespace rgf
