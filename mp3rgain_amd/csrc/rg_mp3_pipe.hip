// rg_mp3_pipe.hip -- the loader pipeline of tuning key 6 = 3 (the default; overview and types: rg_files.h), album parts, and
// the folds of rg_analyze_albums' batches into their albums' packs.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "../../include/mp3rgain_amd_mp4.h"
#include "rg_albums.h"
#include "rg_files.h"
#include "rg_pipe_plan.h"

namespace rgf {

int fold_init(rg_ctx *c, AlbumFold *f) {
    RG_HIP(c, rg_sync_slots(c, RG_SLOT_STREAMS));
    hipStream_t s = c->slots[0].stream;
    RG_HIP(c, hipMemsetAsync(f->d_packs, 0, f->n_packs * (size_t)RG_ALBUMS_PACK_STRIDE * sizeof(uint32_t), s));
    if (f->carried)
        RG_HIP(c, hipMemcpyAsync(f->d_packs, f->d_packs - RG_ALBUMS_PACK_STRIDE, (size_t)RG_ALBUMS_PACK_STRIDE * sizeof(uint32_t),
                                 hipMemcpyDeviceToDevice, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

int fold_batch(rg_ctx *c, AlbumFold *f, const size_t *files, size_t k, hipStream_t s) {
    if (k == 0) return RG_OK;
    if (f->map_used + k > c->h_albums_map.cap || f->map_used + k > c->d_albums_map.cap)
        return rg_set_err(c, RG_ERR_STATE, "rg_analyze_albums: more folded tracks than the group has files");
    int32_t *h = c->h_albums_map.p + f->map_used;
    for (size_t j = 0; j < k; ++j) h[j] = f->pack_of[files[j]];
    int32_t *d = c->d_albums_map.p + f->map_used;
    RG_HIP(c, hipMemcpyAsync(d, h, k * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RgSlot &S = c->slot();
    RG_HIP(c, rg_launch_album_fold(S.d_hist.p, S.peak_ptr, d, (uint32_t)k, f->d_packs, s));
    f->map_used += k;
    return RG_OK;
}

Mp3Pipe &mp3_pipe(rg_ctx *c) {
    if (!c->mp3_pipe) {
        c->mp3_pipe = new Mp3Pipe();
        c->mp3_pipe_free = [](void *p) { delete static_cast<Mp3Pipe *>(p); };
    }
    return *static_cast<Mp3Pipe *>(c->mp3_pipe);
}

}  // namespace rgf

namespace {
using namespace rgf;

constexpr size_t kPipeStageBytes = (size_t)128 << 20;  // staging block (a 3-minute 320 kb/s file is 7.2 MB and 27 600 granule-channels)

struct PipeChunk {
    int stage = 0;
    size_t used = 0;
    uint64_t units = 0;
    std::vector<size_t> files;
    int pending = 0;  // files still being copied into the block
    bool closed = false, issued = false;
};
struct PipeFile {
    StreamLayout at{};  // in its chunk's staging block
    uint64_t main_len = 0;
    uint32_t n_frames = 0;
};

bool read_whole_file(const char *path, Mp3Scratch *sc, size_t *len) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return false;
    struct stat st;
    size_t want = (fstat(fd, &st) == 0 && st.st_size > 0) ? (size_t)st.st_size : 0;
    size_t got = 0;
    for (;;) {
        if (sc->cap < got + 65536 + 64 || sc->cap < want + 64) {
            size_t cap = std::max(std::max(sc->cap * 2, want + 64 + 65536), (size_t)1 << 20);
            uint8_t *q = static_cast<uint8_t *>(realloc(sc->p, cap));
            if (!q) { close(fd); return false; }
            sc->p = q;
            sc->cap = cap;
        }
        const ssize_t k = read(fd, sc->p + got, sc->cap - 64 - got);
        if (k < 0) {
            if (errno == EINTR) continue;
            close(fd);
            return false;
        }
        if (k == 0) break;
        got += (size_t)k;
    }
    close(fd);
    memset(sc->p + got, 0, 64);
    *len = got;
    return true;
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One call of the pipeline.  Built per call on the caller's stack, never copied.  The calling thread is the DRIVE thread
// (prepare, drive, issue, analyze_part, finish: every HIP enqueue of the call); `workers` LOADER threads run loader().
//
// Who may touch what:
//   * guarded by `m`: chunks (and every member of a PipeChunk), open, preparing, files_done, hip_error / hip_msg, starved,
//     tapering, files_placed, units_placed.  `chunks` is a deque: a PipeChunk* stays valid across emplace_back, so the drive
//     thread and a copying loader keep theirs with the lock released.  Once a chunk is closed with pending == 0 nothing but
//     the drive thread touches it, which is what lets issue() and analyze_part() read it unlocked.
//   * the drive thread's alone: arena_used, *parts, the context's enqueue state.
//   * written by exactly one loader, the one that drew file i from next_file: (*out)[i], (*rcs)[i], (*errs)[i], pf[i] and
//     its own P.scratch[w].  The drive thread reads them only for the files of a closed chunk (the lock orders the two), or
//     after the loaders have been joined.
//   * fixed once prepare() has returned: everything else (fs, stage_want, workers, cmd, ...); the trace sums are atomics.
// Outside the lock, always: waiting for a staging block's event and pinning memory (place), the copy into the block
// (load_file), issue() and analyze_part().  cv is notified whenever a loader or the drive thread may have something to do:
// a chunk closed, opened or issued, a copy finished, a file done, a loader giving up.
class PipeCall {
public:
    PipeCall(rg_ctx *c, const char *const *paths, size_t n, std::vector<LoadedAudio> *out, std::vector<int> *rcs, std::vector<std::string> *errs,
             const LoadOpts &opts, PartsRun *parts)
        : c(c), P(mp3_pipe(c)), paths(paths), n(n), out(out), rcs(rcs), errs(errs), opts(opts), parts(parts), pf(n) {}
    int run();

private:
    rg_ctx *const c;
    Mp3Pipe &P;
    const char *const *const paths;
    const size_t n;
    std::vector<LoadedAudio> *const out;
    std::vector<int> *const rcs;
    std::vector<std::string> *const errs;
    const LoadOpts opts;  // the call's own copy: the loader threads read it
    PartsRun *const parts;
    std::vector<PipeFile> pf;
    // fixed by prepare()
    unsigned workers = 0;
    hipStream_t fs = nullptr;
    size_t stage_want = 0;
    bool trace = false;
    double t_start = 0.0, copy_bound_at = 0.0;
    std::string cmd;  // the decoder command, empty where the call's options withhold it
    int flac_route = 0, device = 0;
    // shared
    std::atomic<size_t> next_file{0};
    std::atomic<uint64_t> t_read{0}, t_compact{0}, t_wait{0}, t_copy{0};  // trace: microseconds summed over the loader threads
    std::mutex m;
    std::condition_variable cv;
    // guarded by m
    std::deque<PipeChunk> chunks;
    int open = -1;
    bool preparing = false;  // a loader is getting the next chunk's staging block ready, outside the lock
    size_t files_done = 0;
    int hip_error = RG_OK;
    std::string hip_msg;
    bool starved = false;       // the device was found idle when the latest chunk became ready: the host's loaders are the longer stage
    bool tapering = false;      // the call's last chunks are being made smaller
    size_t files_placed = 0;    // files that have their place in a chunk
    uint64_t units_placed = 0;
    // the drive thread's
    size_t arena_used = 0;

    void hip_fail(const char *what) {  // m held
        if (hip_error == RG_OK) { hip_error = RG_ERR_DEVICE; hip_msg = what; }
    }
    bool ready(size_t k) const { return k < chunks.size() && chunks[k].closed && chunks[k].pending == 0; }  // m held
    int prepare();
    bool classify(size_t i, Mp3Scratch &sc, uint64_t *units, double *tl);
    PipeChunk *place(size_t i, const Mp3Scratch &sc, uint64_t units, uint8_t **dst);
    void load_file(size_t i, Mp3Scratch &sc);
    void loader(unsigned w);
    int issue(PipeChunk &ch, size_t index);
    int analyze_part(const PipeChunk *ch, size_t index, bool last, bool starved_now);
    int drive();
    int finish();
};

int PipeCall::prepare() {
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    workers = c->loader_threads ? c->loader_threads : usable_cores();
    if (workers > n) workers = (unsigned)n;
    if (P.scratch.size() < workers) P.scratch.resize(workers);
    for (Mp3Stage &st : P.stage)
        if (!st.staged) RG_HIP(c, hipEventCreateWithFlags(&st.staged, hipEventDisableTiming));
    // earlier batches may still read the arena and the chunk buffers
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    // The decode runs on the FIRST pipeline stream, whichever slot the last batch used, and the copies on the second
    // (rg_mp3dev_enqueue_chunk): the runtime maps streams onto four hardware queues, and with a fifth stream for the copies and
    // the decode on "the current slot's stream" every fourth call landed on the queue the copy stream shared and took 25 instead
    // of 20 ms (tools/seq_album.py).
    fs = c->user_attached ? c->user_stream : c->slots[0].stream;
    if (parts) {  // decode and parts share that stream: see PartsRun
        RG_HIP(c, hipStreamSynchronize(fs));
        if (P.part_ev.size() < 2 * kMaxParts) {
            const size_t have = P.part_ev.size();
            P.part_ev.resize(2 * kMaxParts, nullptr);
            for (size_t k = have; k < P.part_ev.size(); ++k) RG_HIP(c, hipEventCreateWithFlags(&P.part_ev[k], hipEventDisableTiming));
        }
        RG_HIP(c, c->h_mp3_part_counts.reserve(n * kMaxParts));
        RG_HIP(c, c->h_part_results.reserve(n));
        if (parts->album) RG_HIP(c, c->d_album_packs.reserve(kMaxParts * (size_t)RG_ALBUM_PACK_WORDS));
    }
    rc = rg_mp3dev_reserve_results(c, n, fs);
    if (rc != RG_OK) return rc;

    trace = c->trace_files;
    t_start = now();
    {   // staging blocks no larger than the call needs: a single album of a dozen files should not pin 3 x 96 MB
        size_t total = 0;
        for (size_t i = 0; i < n; ++i) {
            struct stat st;
            if (paths[i] && stat(paths[i], &st) == 0 && st.st_size > 0) total += (size_t)st.st_size;
        }
        size_t cap = kPipeStageBytes;
        if (c->stage_bytes()) cap = c->stage_bytes();  // tests: tiny blocks, so that a handful of small files exercises the whole rotation
        stage_want = std::min(cap, total + total / 8 + ((size_t)1 << 16));
    }
    if (opts.decoder_command) cmd = c->decoder_cmd;
    flac_route = c->gpu_flac_decode;
    device = c->device;
    copy_bound_at = parts ? c->parts_min_bpu() : 0.0;
    return RG_OK;
}

// File i is read into `sc`.  What is not a bare MPEG stream ends here, loaded as load_audio_for loads it or with its error;
// an MPEG stream is compacted in `sc` and described in (*out)[i] and pf[i]: true, and its granule-channels in *units.
bool PipeCall::classify(size_t i, Mp3Scratch &sc, uint64_t *units, double *tl) {
    LoadedAudio &la = (*out)[i];
    std::string &err = (*errs)[i];
    const char *path = paths[i];
    char msg[1024];
    if (!path) { (*rcs)[i] = RG_ERR_INVALID_ARG; err = "null path"; return false; }
    size_t len = 0;
    tl[0] = trace ? now() : 0.0;
    if (!read_whole_file(path, &sc, &len)) {
        snprintf(msg, sizeof msg, "Failed to open: %s", path);  // src/replaygain.rs:804-805
        (*rcs)[i] = RG_ERR_IO;
        err = msg;
        return false;
    }
    if (len >= 12 && memcmp(sc.p, "RIFF", 4) == 0 && memcmp(sc.p + 8, "WAVE", 4) == 0) {
        la.wav.assign(sc.p, sc.p + len);
        return false;
    }
    if (rg_flac_is_flac(sc.p, len)) {  // (before the MPEG probe, as in load_audio_for)
        la.file_bytes.assign(sc.p, sc.p + len);
        const int frc = load_flac(flac_route, path, &la, &err);
        if (frc != kFlacNotHere) {
            (*rcs)[i] = frc;
            return false;
        }
        la.kind = LoadedAudio::Wav;
        (*rcs)[i] = cmd.empty() ? RG_ERR_FORMAT : load_audio_for(cmd, 2, path, &la, &err, opts.track_index, flac_route);
        return false;
    }
    const bool mp4 = len >= 8 && memcmp(sc.p + 4, "ftyp", 4) == 0;
    la.is_mp4 = rg_mp4_is_mp4_data(sc.p, len) != 0;
    rg_mp3_stream_info si;
    uint64_t main_len = 0;
    tl[1] = trace ? now() : 0.0;
    if (opts.keep_mpeg_bytes && !mp4) la.file_bytes.assign(sc.p, sc.p + len);  // rg_mp3_verify: the compaction below works in place
    if (mp4 || rg_mp3_compact_stream(sc.p, len, &sc.slots, &sc.tiles, &main_len, &si) != RG_MP3DEC_OK || si.audio_frames == 0) {
        (*rcs)[i] = load_audio_for(cmd, 2, path, &la, &err, opts.track_index, flac_route);  // the decoder command, or the reference's probe error
        return false;
    }
    la.sample_rate = si.sample_rate;
    la.channels = si.channels;
    la.lsf = si.mpeg_version == 1 ? 0u : 1u;
    la.walked_frames = si.frames;
    la.frames = si.frames;
    la.result_index = (uint32_t)i;
    la.kind = LoadedAudio::Staged;
    *units = (uint64_t)si.audio_frames * (la.lsf ? 1u : 2u) * si.channels;
    pf[i].main_len = main_len;
    pf[i].n_frames = si.audio_frames;
    return true;
}

// A place for file i's compacted stream (in `sc`, `units` granule-channels): the open chunk if it has room, else that one
// closes and the next opens as soon as a staging block is free.  Returns the chunk (its `pending` counts this file until the
// copy is done) with pf[i].at set and *dst its block; or null: no pinned memory, the file carries the error.
PipeChunk *PipeCall::place(size_t i, const Mp3Scratch &sc, uint64_t units, uint8_t **dst) {
    const size_t slot_bytes = sc.slots.size(), tile_bytes = sc.tiles.size() * sizeof(uint64_t);
    const size_t need = stream_layout(0, (size_t)pf[i].main_len, slot_bytes, tile_bytes).end;
    auto no_memory = [&] {  // m held
        hip_fail("hipHostMalloc of a staging block failed");
        (*rcs)[i] = RG_ERR_DEVICE;
        (*errs)[i] = "out of pinned memory";
        (*out)[i].kind = LoadedAudio::Wav;
    };
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
        if (open >= 0) {
            PipeChunk &ch = chunks[(size_t)open];
            Mp3Stage &st = P.stage[ch.stage];
            const size_t with = ch.used + need + rg_mp3dev_track_bytes(ch.files.size() + 1) + 64;
            const uint64_t unit_cap = rg_pipe_unit_cap((size_t)open, ch.units, starved, files_placed, units_placed, n, &tapering);
            if (with <= st.cap && ch.units + units <= unit_cap) break;
            if (ch.files.empty()) {  // a stream larger than a block: the block grows (nothing is in flight from it)
                if (st.grow(with) != hipSuccess) { no_memory(); return nullptr; }
                break;
            }
            ch.closed = true;
            open = -1;
            cv.notify_all();
        }
        const size_t id = chunks.size();
        // every block is filling or waiting to be sent, or another loader is already preparing the next one
        if (preparing || (id >= (size_t)Mp3Pipe::NSTAGE && !chunks[id - Mp3Pipe::NSTAGE].issued)) {
            cv.wait(lk);
            continue;
        }
        // Waiting for the block's last H2D copy and pinning memory (up to 128 MB) happen WITHOUT the lock: every
        // loader and the drive thread take it for each file and each chunk, and one loader sitting on it stalled
        // file reads, copy completion and chunk issue for all the others.
        Mp3Stage &st = P.stage[id % Mp3Pipe::NSTAGE];
        preparing = true;
        lk.unlock();
        bool ev_ok = true, mem_ok = true;
        if (id >= (size_t)Mp3Pipe::NSTAGE) {
            (void)hipSetDevice(device);
            ev_ok = hipEventSynchronize(st.staged) == hipSuccess;
        }
        mem_ok = st.grow(std::max(stage_want, (size_t)4096)) == hipSuccess;
        lk.lock();
        preparing = false;
        if (!ev_ok) hip_fail("waiting for a staging block failed");
        if (!mem_ok) {
            no_memory();
            cv.notify_all();
            return nullptr;
        }
        chunks.emplace_back();
        chunks.back().stage = (int)(id % Mp3Pipe::NSTAGE);
        open = (int)id;
        cv.notify_all();
    }
    PipeChunk *chunk = &chunks[(size_t)open];
    pf[i].at = stream_layout(chunk->used, (size_t)pf[i].main_len, slot_bytes, tile_bytes);
    chunk->used = pf[i].at.end;
    chunk->units += units;
    files_placed++;
    units_placed += units;
    chunk->files.push_back(i);
    chunk->pending++;
    *dst = P.stage[chunk->stage].p;
    return chunk;
}

void PipeCall::load_file(size_t i, Mp3Scratch &sc) {
    double tl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // trace: before the read, the compaction, the wait for a place, the copy, and after it
    uint64_t units = 0;
    if (!classify(i, sc, &units, tl)) return;
    tl[2] = trace ? now() : 0.0;
    uint8_t *dst = nullptr;
    PipeChunk *chunk = place(i, sc, units, &dst);
    if (!chunk) return;
    tl[3] = trace ? now() : 0.0;
    copy_stream_into(dst, pf[i].at, sc, (size_t)pf[i].main_len);
    if (trace) {
        tl[4] = now();
        t_read += (uint64_t)((tl[1] - tl[0]) * 1e6);
        t_compact += (uint64_t)((tl[2] - tl[1]) * 1e6);
        t_wait += (uint64_t)((tl[3] - tl[2]) * 1e6);
        t_copy += (uint64_t)((tl[4] - tl[3]) * 1e6);
    }
    {
        std::lock_guard<std::mutex> lk(m);
        chunk->pending--;
    }
    cv.notify_all();
}

void PipeCall::loader(unsigned w) {
    (void)hipSetDevice(device);  // the staging blocks a loader allocates or waits for belong to this context's GPU
    for (size_t i = next_file.fetch_add(1); i < n; i = next_file.fetch_add(1)) {
        load_file(i, P.scratch[w]);
        {
            std::lock_guard<std::mutex> lk(m);
            files_done++;
        }
        cv.notify_all();
    }
}

// ---- the calling thread: send chunks as they close ---------------------------------------------------------------
int PipeCall::issue(PipeChunk &ch, size_t index) {
    std::vector<RgMp3StreamItem> items(ch.files.size());
    size_t top = arena_used;
    for (size_t k = 0; k < ch.files.size(); ++k) {
        LoadedAudio &la = (*out)[ch.files[k]];
        la.arena_off = top;
        top = align16(top + (size_t)la.walked_frames * la.channels * sizeof(float));
    }
    int r = arena_reserve_keep(c, top ? top : 16, arena_used);
    if (r != RG_OK) return r;
    arena_used = top;
    for (size_t k = 0; k < ch.files.size(); ++k) {
        const size_t i = ch.files[k];
        const LoadedAudio &la = (*out)[i];
        items[k] = stream_item(pf[i].at, pf[i].n_frames, la.channels, la.sample_rate, la.lsf, la.result_index, c->d_arena.p + la.arena_off);
    }
    Mp3Stage &st = P.stage[ch.stage];
    const size_t tracks_off = (ch.used + 7) & ~(size_t)7;
    if (parts && index >= kMaxParts) parts->broken = true;
    const bool part = parts && !parts->broken;
    r = rg_mp3dev_enqueue_chunk(c, (int)(index & 1), st.p, tracks_off + rg_mp3dev_track_bytes(items.size()), tracks_off, st.staged,
                                items.data(), items.size(), fs, part ? c->h_mp3_part_counts.p + index * n : nullptr, n,
                                part ? P.part_ev[2 * index + 1] : nullptr);
    if (r == RG_OK && part) RG_HIP(c, hipEventRecord(P.part_ev[2 * index], fs));
    return r;
}

// the tracks of chunk `index` (decode enqueued, the chunk after it too) as one part of the album
// `ch` (may be null: nothing new) joins what is pending; `index`: the newest chunk whose files are pending or were
// `starved_now`: when the chunk after `ch` was ready to be sent, the device had already finished `ch`'s decode, i.e. it is the
// host's loaders the call is waiting for (few of them: one loader thread reads and walks 6 GB/s of VBR files, the device
// takes 17): the analysis of the files so far costs nothing while it waits.
int PipeCall::analyze_part(const PipeChunk *ch, size_t index, bool last, bool starved_now) {
    if (!parts || parts->broken) return RG_OK;
    bool copy_bound = false;
    if (ch) {
        parts->pending.insert(parts->pending.end(), ch->files.begin(), ch->files.end());
        copy_bound = rg_pipe_chunk_is_part(ch->used, ch->units, copy_bound_at, starved_now);
    }
    if (!copy_bound && !(last && parts->n_parts)) {
        if (last) parts->broken = true;  // no chunk of the album was copy-bound: the plain route, one launch over all of it
        return RG_OK;
    }
    if (parts->pending.empty()) return RG_OK;
    std::vector<size_t> files;
    files.swap(parts->pending);
    RG_HIP(c, hipEventSynchronize(P.part_ev[2 * index + 1]));  // the frame parser ran at the head of the chunk's work: long done
    const uint32_t *counts = c->h_mp3_part_counts.p + index * n;  // (the counts of every earlier chunk are in this copy as well)
    std::vector<rg_track_desc> descs(files.size());
    for (size_t k = 0; k < files.size(); ++k) {
        const size_t i = files[k];
        LoadedAudio &la = (*out)[i];
        std::string msg;
        if (la.kind != LoadedAudio::Staged || file_outcome(la, (*rcs)[i], (*errs)[i], paths[i], opts.track_index, &msg) != RG_OK) {
            parts->broken = true;  // the plain route reports it, in input order
            return RG_OK;
        }
        rg_track_desc &d = descs[k];
        d = rg_track_desc{};
        d.offset_bytes = la.arena_off;
        d.frames = (uint64_t)counts[la.result_index] * 576;
        d.sample_rate = la.sample_rate;
        d.channels = (uint16_t)la.channels;
        d.format = RG_FMT_F32_PLANAR;
    }
    // on the decode's stream (behind the decode of the chunk after this part's), with the buffers of the next pipeline slot:
    // one batch in flight at a time (cost model: one_shot); with three or more slots (the callers' condition for parts) the
    // slot taken here had its last descriptor copy two parts ago, so its pinned descriptors are not waited for
    c->enqueue_wait_ev = P.part_ev[2 * index];
    c->enqueue_stream = fs;
    const bool one_shot_before = c->one_shot;
    c->one_shot = true;
    const int r = rg_enqueue_impl(c, descs.data(), descs.size(), c->d_arena.p, arena_used, parts->album);
    c->one_shot = one_shot_before;
    c->enqueue_stream = nullptr;
    c->enqueue_wait_ev = nullptr;
    if (r != RG_OK) {
        parts->broken = true;
        return RG_OK;
    }
    RgSlot &S = c->slot();
    if (parts->album)
        RG_HIP(c, hipMemcpyAsync(c->d_album_packs.p + parts->n_parts * (size_t)RG_ALBUM_PACK_WORDS, S.d_album_hist.p,
                                 (size_t)RG_ALBUM_PACK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, fs));
    RG_HIP(c, hipMemcpyAsync(c->h_part_results.p + parts->file_of.size(), S.d_results.p, descs.size() * sizeof(rg_track_result),
                             hipMemcpyDeviceToHost, fs));
    if (parts->fold) {  // (before the slot's accumulators serve a later part: same stream)
        const int fr = fold_batch(c, parts->fold, files.data(), files.size(), fs);
        if (fr != RG_OK) return fr;
    }
    parts->n_parts++;
    parts->file_of.insert(parts->file_of.end(), files.begin(), files.end());
    return RG_OK;
}

int PipeCall::drive() {
    int result = RG_OK;
    size_t next = 0;
    const PipeChunk *prev = nullptr;  // issued, not yet analysed as a part
    size_t prev_index = 0;
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
        cv.wait(lk, [&] { return ready(next) || files_done == n; });
        if (!ready(next)) {
            if (open >= 0) {  // every file is in: the last chunk closes as it is
                chunks[(size_t)open].closed = true;
                open = -1;
                continue;
            }
            if (next >= chunks.size()) {
                if (result == RG_OK && parts) {
                    lk.unlock();
                    const int r = analyze_part(prev, prev_index, true, false);
                    lk.lock();
                    if (r != RG_OK) result = r;
                    prev = nullptr;
                }
                break;
            }
            continue;
        }
        PipeChunk &ch = chunks[next];
        const size_t done_now = files_done;
        lk.unlock();
        const double t_i = now();
        const bool observed = parts && !parts->broken && prev && c->parts_when_starved();
        const bool starved_now = observed && hipEventQuery(P.part_ev[2 * prev_index]) == hipSuccess;
        int r = (result == RG_OK && !ch.files.empty()) ? issue(ch, next) : RG_OK;
        if (r == RG_OK && result == RG_OK && prev) {  // the device has this chunk's decode to go on with
            r = analyze_part(prev, prev_index, false, starved_now);
            prev = nullptr;
        }
        if (r == RG_OK && result == RG_OK && !ch.files.empty()) {
            prev = &ch;
            prev_index = next;
        }
        if (trace)
            fprintf(stderr, "[pipeline] chunk %zu: %zu files, %.1f MB, %llu units, ready at %.1f ms (files done %zu)%s, enqueue took %.2f ms\n", next,
                    ch.files.size(), ch.used / 1e6, (unsigned long long)ch.units, (t_i - t_start) * 1e3, done_now, starved_now ? ", the device was idle" : "",
                    (now() - t_i) * 1e3);
        lk.lock();
        if (observed && !tapering) starved = starved_now;  // the latest finding counts
        if (r != RG_OK && result == RG_OK) result = r;
        if (r != RG_OK || ch.files.empty()) (void)hipEventRecord(P.stage[ch.stage].staged, fs);  // loaders wait on it before refilling the block
        ch.issued = true;
        ++next;
        cv.notify_all();
    }
    return result;
}

// every chunk is enqueued and the loaders are gone: the device's findings, how much of each stream decoded
int PipeCall::finish() {
    if (hip_error != RG_OK) return rg_set_err(c, hip_error, "%s", hip_msg.c_str());
    const double t_issued = now();
    int rc = rg_mp3dev_fetch_results(c, n, fs);
    if (rc != RG_OK) return rc;
    RG_HIP(c, hipStreamSynchronize(fs));
    if (trace)
        fprintf(stderr, "[pipeline] all chunks enqueued at %.1f ms, device done at %.1f ms; %u loader threads, summed: read %.1f ms, compact %.1f ms, "
                        "waiting for a block %.1f ms, copy into the block %.1f ms\n", (t_issued - t_start) * 1e3, (now() - t_start) * 1e3, workers,
                t_read.load() / 1e3, t_compact.load() / 1e3, t_wait.load() / 1e3, t_copy.load() / 1e3);
    const uint32_t *granules = rg_mp3dev_results(c);
    for (size_t i = 0; i < n; ++i) {
        LoadedAudio &la = (*out)[i];
        if (la.kind == LoadedAudio::Staged) la.frames = (uint64_t)granules[la.result_index] * 576;
    }
    if (!c->user_attached) RG_HIP(c, hipEventRecord(c->user_ev, fs));
    c->user_dirty = true;
    return RG_OK;
}

int PipeCall::run() {
    int rc = prepare();
    if (rc != RG_OK) return rc;
    if (n == 1) {  // one stream is one chunk: nothing to overlap
        loader(0);
        rc = drive();
    } else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w) pool.emplace_back(&PipeCall::loader, this, w);
        rc = drive();
        for (auto &t : pool) t.join();
    }
    return rc != RG_OK ? rc : finish();
}

}  // namespace

int rgf::pipe_load_many(rg_ctx *c, const char *const *paths, size_t n, std::vector<LoadedAudio> *out, std::vector<int> *rcs,
                        std::vector<std::string> *errs, const LoadOpts &opts, PartsRun *parts) {
    return PipeCall(c, paths, n, out, rcs, errs, opts, parts).run();
}
