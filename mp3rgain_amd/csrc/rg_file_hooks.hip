// rg_file_hooks.hip -- measurement and parity hooks of the file layer's device decoders: one stream in memory through the
// decode chain, timed (rg_mp3_decode_bench) or with the PCM brought back (rg_mp3_decode_device, rg_flac_decode_device), and
// a batch of FLAC streams through the file route's staging with the arena brought back (rg_flac_stage_device_batch).
#include <new>
#include <string>
#include <vector>

#include "rg_files.h"

using namespace rgf;

// One MPEG Layer III stream in memory into the context's first scratch buffer, compacted there as the loader pipeline's
// loaders compact a file (rg_mp3_pipe.hip): *sc_out holds main data, slots and tiles, *main_len and *si describe them.
static int compact_into_scratch(rg_ctx *c, const void *data, size_t len, Mp3Scratch **sc_out, uint64_t *main_len, rg_mp3_stream_info *si) {
    Mp3Pipe &P = mp3_pipe(c);
    if (P.scratch.empty()) P.scratch.resize(1);
    Mp3Scratch &sc = P.scratch[0];
    if (!sc.reserve(len)) return rg_set_err(c, RG_ERR_IO, "out of memory");
    memcpy(sc.p, data, len);
    memset(sc.p + len, 0, 64);
    if (rg_mp3_compact_stream(sc.p, len, &sc.slots, &sc.tiles, main_len, si) != RG_MP3DEC_OK)
        return rg_set_err(c, RG_ERR_FORMAT, "%s", rg_mp3dec_last_error());
    *sc_out = &sc;
    return RG_OK;
}

// Measurement hook (bench.py, tools/): the device decode chain alone.  `copies` copies of one MPEG Layer III stream form ONE
// chunk of the default route (compacted by the host once, staged in pinned memory, copied H2D per repetition on the copy
// stream), and the chunk's three stages -- frame parser (three launches), Huffman, back half -- are bracketed with HIP events
// on the stream they run on.  ms_out[0..2] = average duration of each stage over `reps` repetitions, ms_out[3] = first event
// to last (the chain), ms_out[4] = per chunk in the file route's own arrangement (parser and sort beside the chunk before);
// the PCM lands in the analysis arena as in a real call and is not copied back.
extern "C" int rg_mp3_decode_bench(rg_ctx *c, const void *data, size_t len, uint32_t copies, uint32_t reps, double *ms_out /* 5 */,
                                   uint64_t *units_out, uint64_t *compressed_bytes_out, uint64_t *frames_out) {
    if (!c || !data || !ms_out || copies == 0 || reps == 0) return RG_ERR_INVALID_ARG;
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    Mp3Scratch *scp = nullptr;
    rg_mp3_stream_info si;
    uint64_t main_len = 0;
    rc = compact_into_scratch(c, data, len, &scp, &main_len, &si);
    if (rc != RG_OK) return rc;
    const Mp3Scratch &sc = *scp;
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    const size_t per_stream = (size_t)si.frames * si.channels * sizeof(float);
    RG_HIP(c, c->d_arena.reserve(per_stream * copies + 64));
    const size_t slot_bytes = sc.slots.size(), tile_bytes = sc.tiles.size() * sizeof(uint64_t);
    const size_t one = stream_layout(0, (size_t)main_len, slot_bytes, tile_bytes).end;
    const size_t tracks_off = one * copies;
    const size_t total = tracks_off + rg_mp3dev_track_bytes(copies);
    Mp3Stage &st = mp3_pipe(c).stage[0];
    if (!st.staged) RG_HIP(c, hipEventCreateWithFlags(&st.staged, hipEventDisableTiming));
    RG_HIP(c, st.grow(total));
    std::vector<RgMp3StreamItem> items(copies);
    for (uint32_t k = 0; k < copies; ++k) {
        const StreamLayout at = stream_layout(one * k, (size_t)main_len, slot_bytes, tile_bytes);
        copy_stream_into(st.p, at, sc, (size_t)main_len);
        items[k] = stream_item(at, si.audio_frames, si.channels, si.sample_rate, si.mpeg_version == 1 ? 0u : 1u, k, c->d_arena.p + per_stream * k);
    }
    hipStream_t fs = c->slots[0].stream;  // as the file route: never the stream the copies run on (rg_mp3dev_enqueue_chunk)
    // one set of events per repetition: the repetitions are enqueued back to back (a synchronise after each would let the
    // clocks fall between them) and read out at the end
    if (reps > 256) reps = 256;
    std::vector<hipEvent_t> ev((size_t)4 * (reps + 1), nullptr);
    for (hipEvent_t &e : ev) RG_HIP(c, hipEventCreate(&e));
    double sum[4] = {0, 0, 0, 0};
    rc = rg_mp3dev_reserve_results(c, copies, fs);
    for (uint32_t r = 0; r < reps + 1 && rc == RG_OK; ++r) {  // the first repetition is not counted
        c->mp3_bench_ev = &ev[(size_t)4 * r];
        rc = rg_mp3dev_enqueue_chunk(c, (int)(r & 1), st.p, total, tracks_off, st.staged, items.data(), copies, fs);
        c->mp3_bench_ev = nullptr;
    }
    if (rc == RG_OK && hipStreamSynchronize(fs) != hipSuccess) rc = rg_set_err(c, RG_ERR_DEVICE, "decode bench: stream synchronise failed");
    for (uint32_t r = 1; r < reps + 1 && rc == RG_OK; ++r) {
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, ev[(size_t)4 * r + k], ev[(size_t)4 * r + k + 1]);
            sum[k] += ms;
        }
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ev[(size_t)4 * r], ev[(size_t)4 * r + 3]);
        sum[3] += ms;
    }
    // The production arrangement: the same chunk `reps` times the way the file route enqueues chunks -- frame parser and lane
    // sort on the copy stream behind the chunk's H2D, i.e. beside the Huffman / back-half kernels of the chunk before -- first
    // event to last on the chain's stream, per chunk (the first chunk's parser has nothing to run beside: 1 / reps of the figure).
    double piped = 0.0;
    if (rc == RG_OK) {
        for (uint32_t r = 0; r < reps + 2 && rc == RG_OK; ++r) {
            if (r == 2) rc = hipEventRecord(ev[0], fs) == hipSuccess ? RG_OK : RG_ERR_DEVICE;  // two chunks ahead: the pipeline is full
            if (rc == RG_OK) rc = rg_mp3dev_enqueue_chunk(c, (int)(r & 1), st.p, total, tracks_off, st.staged, items.data(), copies, fs);
        }
        if (rc == RG_OK && (hipEventRecord(ev[1], fs) != hipSuccess || hipStreamSynchronize(fs) != hipSuccess))
            rc = rg_set_err(c, RG_ERR_DEVICE, "decode bench: stream synchronise failed");
        float ms = 0.0f;
        if (rc == RG_OK) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        piped = (double)ms / reps;
    }
    for (hipEvent_t &e : ev) (void)hipEventDestroy(e);
    if (rc != RG_OK) return rc;
    for (int k = 0; k < 4; ++k) ms_out[k] = sum[k] / reps;
    ms_out[4] = piped;
    const uint64_t per_frame = si.mpeg_version == 1 ? 2u : 1u;
    if (units_out) *units_out = (uint64_t)si.audio_frames * per_frame * si.channels * copies;
    if (compressed_bytes_out) *compressed_bytes_out = (uint64_t)(main_len + sc.slots.size()) * copies;
    if (frames_out) *frames_out = (uint64_t)si.frames * copies;
    return RG_OK;
}

// Decode one MPEG Layer III stream through the split decoder (stage A on the host, B-E on the device) and bring the PCM
// back: the parity hook of tests/test_gpu_mp3.py.  Same outputs as rg_mp3_decode_f32.
extern "C" int rg_mp3_decode_device(rg_ctx *c, const void *data, size_t len, float *ch0, float *ch1, uint64_t capacity,
                                    void *info) {
    rg_mp3_stream_info *out = static_cast<rg_mp3_stream_info *>(info);
    if (!c || !data || !out || !ch0) return RG_ERR_INVALID_ARG;
    if (c->gpu_mp3_decode >= 3) {  // the default route: the host strips headers and side information, nothing else
        int rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        Mp3Scratch *sc = nullptr;
        uint64_t main_len = 0;
        rc = compact_into_scratch(c, data, len, &sc, &main_len, out);
        if (rc != RG_OK) return rc;
        if (out->frames > capacity) return rg_set_err(c, RG_ERR_INVALID_ARG, "capacity %llu < %llu frames", (unsigned long long)capacity, (unsigned long long)out->frames);
        if (out->channels == 2 && !ch1) return rg_set_err(c, RG_ERR_INVALID_ARG, "stereo stream needs a second output channel");
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        const size_t bytes = (size_t)out->frames * out->channels * sizeof(float);
        RG_HIP(c, c->d_arena.reserve(bytes ? bytes : 16));
        Mp3Stage &st = mp3_pipe(c).stage[0];
        if (!st.staged) RG_HIP(c, hipEventCreateWithFlags(&st.staged, hipEventDisableTiming));
        const StreamLayout at = stream_layout(0, (size_t)main_len, sc->slots.size(), sc->tiles.size() * sizeof(uint64_t));
        const size_t tracks_off = at.end;
        const size_t total = tracks_off + rg_mp3dev_track_bytes(1);
        RG_HIP(c, st.grow(total));
        copy_stream_into(st.p, at, *sc, (size_t)main_len);
        const RgMp3StreamItem it = stream_item(at, out->audio_frames, out->channels, out->sample_rate, out->mpeg_version == 1 ? 0u : 1u, 0, c->d_arena.p);
        hipStream_t fs = c->slots[0].stream;
        rc = rg_mp3dev_reserve_results(c, 1, fs);
        if (rc != RG_OK) return rc;
        rc = rg_mp3dev_enqueue_chunk(c, 0, st.p, total, tracks_off, st.staged, &it, 1, fs);
        if (rc != RG_OK) return rc;
        rc = rg_mp3dev_fetch_results(c, 1, fs);
        if (rc != RG_OK) return rc;
        RG_HIP(c, hipStreamSynchronize(fs));
        const uint32_t granules = rg_mp3dev_results(c)[0];
        const uint32_t per_frame = it.lsf ? 1u : 2u;
        const uint32_t walked = out->audio_frames;
        out->frames = (uint64_t)granules * 576;
        out->audio_frames = granules / per_frame;
        out->skipped_frames = walked - out->audio_frames;
        if (out->frames) {
            RG_HIP(c, hipMemcpy(ch0, it.d_ch0, (size_t)out->frames * sizeof(float), hipMemcpyDeviceToHost));
            if (out->channels == 2) RG_HIP(c, hipMemcpy(ch1, it.d_ch0 + out->frames, (size_t)out->frames * sizeof(float), hipMemcpyDeviceToHost));
        }
        return RG_OK;
    }
    rg_mp3_stream_info si;
    if (rg_mp3_scan(data, len, &si) != RG_MP3DEC_OK) return rg_set_err(c, RG_ERR_FORMAT, "%s", rg_mp3dec_last_error());
    const uint64_t cap = (uint64_t)si.audio_frames * (si.mpeg_version == 1 ? 2u : 1u) * si.channels;
    std::vector<int16_t> is;
    std::vector<rg_mp3_unit> units;
    std::vector<uint8_t> main_stream;
    std::vector<RgMp3HuffRec> recs;
    uint64_t n_units = 0;
    if (c->gpu_mp3_decode == 2) {
        if (rg_mp3_index_stream(data, len, &main_stream, &recs, out) != RG_MP3DEC_OK)
            return rg_set_err(c, RG_ERR_FORMAT, "%s", rg_mp3dec_last_error());
        n_units = recs.size();
    } else {
        is.resize((size_t)cap * 576 + 1);
        units.resize((size_t)cap + 1);
        if (rg_mp3_parse_units(data, len, is.data(), units.data(), cap, &n_units, out) != RG_MP3DEC_OK)
            return rg_set_err(c, RG_ERR_FORMAT, "%s", rg_mp3dec_last_error());
    }
    if (out->frames > capacity) return rg_set_err(c, RG_ERR_INVALID_ARG, "capacity %llu < %llu frames", (unsigned long long)capacity, (unsigned long long)out->frames);
    if (out->channels == 2 && !ch1) return rg_set_err(c, RG_ERR_INVALID_ARG, "stereo stream needs a second output channel");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    const size_t bytes = (size_t)out->frames * out->channels * sizeof(float);
    RG_HIP(c, c->d_arena.reserve(bytes ? bytes : 16));
    RgMp3SplitItem it{};
    it.is = is.data();
    it.units = units.data();
    if (c->gpu_mp3_decode == 2) {
        it.recs = recs.data();
        it.main = main_stream.data();
        it.main_len = main_stream.size();
    }
    it.n_units = n_units;
    it.channels = out->channels;
    it.rate_row = (uint32_t)rg_mp3_rate_row(out->sample_rate);
    it.lsf = out->mpeg_version == 1 ? 0u : 1u;
    it.d_ch0 = reinterpret_cast<float *>(c->d_arena.p);
    it.d_ch1 = out->channels == 2 ? it.d_ch0 + out->frames : nullptr;
    hipStream_t fs = c->slot().stream;
    rc = rg_mp3dev_decode(c, &it, 1, fs);
    if (rc != RG_OK) return rc;
    if (out->frames) {
        RG_HIP(c, hipMemcpy(ch0, it.d_ch0, (size_t)out->frames * sizeof(float), hipMemcpyDeviceToHost));
        if (out->channels == 2) RG_HIP(c, hipMemcpy(ch1, it.d_ch1, (size_t)out->frames * sizeof(float), hipMemcpyDeviceToHost));
    }
    return RG_OK;
}

// Decode one FLAC stream through the device route's kernels and bring the PCM back, right-justified int32: the parity hook
// of tests/test_gpu_flac.py.  Same outputs as rg_flac_decode_s32.
extern "C" int rg_flac_decode_device(void *ctx, const void *data, size_t len, int32_t *const *planes, uint64_t capacity, rg_flac_info *out) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c || !data || !out || !planes) return RG_ERR_INVALID_ARG;
    std::vector<rg_flac_frame> frames;
    rg_flac_info si;
    if (rg_flac_index_vec((const uint8_t *)data, len, &frames, &si) != RG_FLAC_OK) return rg_set_err(c, RG_ERR_FORMAT, "%s", rg_flac_last_error());
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    const size_t bytes = (size_t)si.frames * si.channels * sizeof(int32_t);
    RG_HIP(c, c->d_arena.reserve(bytes ? bytes : 16));
    RgFlacDevStream st{};
    st.bytes = (const uint8_t *)data;
    st.len = len;
    st.frames = frames.data();
    st.n_frames = (uint32_t)frames.size();
    st.channels = si.channels;
    st.bps = si.bits_per_sample;
    st.elem_bytes = 4;
    st.shift = 0;
    st.dst = c->d_arena.p;
    hipStream_t fs = c->slots[0].stream;
    rc = rg_flacdev_decode(c, &st, 1, fs);
    if (rc != RG_OK) return rc;
    *out = si;
    out->frames = st.samples;
    out->audio_frames = st.decoded_frames;
    out->dropped_frames = st.dropped_frames;
    if (st.samples > capacity) return rg_set_err(c, RG_ERR_INVALID_ARG, "capacity %llu < %llu frames", (unsigned long long)capacity, (unsigned long long)st.samples);
    for (uint32_t ch = 0; ch < si.channels && st.samples; ++ch)
        RG_HIP(c, hipMemcpy(planes[ch], c->d_arena.p + (size_t)ch * st.samples * sizeof(int32_t), (size_t)st.samples * sizeof(int32_t), hipMemcpyDeviceToHost));
    c->user_dirty = true;
    return RG_OK;
}

// `n` FLAC streams in memory through the file route's own loading and staging (load_flac with the context's tuning key 14,
// then stage_loaded: one rg_flacdev_decode for all of them, or the host decoder's repacked PCM), and the arena brought
// back with the track descriptors the analysis kernels would be given: the parity hook of tests/test_gpu_flac_batch.py.
extern "C" int rg_flac_stage_device_batch(void *ctx, size_t n, const void *const *data, const size_t *len, rg_track_desc *descs,
                                          rg_flac_info *infos, void *arena_out, size_t arena_capacity, size_t *arena_bytes) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c || !n || !data || !len || !descs || !infos || !arena_bytes || (arena_capacity && !arena_out)) return RG_ERR_INVALID_ARG;
    try {
        std::vector<LoadedAudio> &pool = file_pool(c, n);
        for (size_t i = 0; i < n; ++i) {
            if (!data[i]) return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: null data", i);
            if (rg_flac_scan(data[i], len[i], &infos[i]) != RG_FLAC_OK) return rg_set_err(c, RG_ERR_FORMAT, "stream %zu: %s", i, rg_flac_last_error());
            const uint8_t *p = static_cast<const uint8_t *>(data[i]);
            pool[i].file_bytes.assign(p, p + len[i]);
            std::string err;
            const std::string name = "stream " + std::to_string(i);
            const int lrc = load_flac(c->gpu_flac_decode, name.c_str(), &pool[i], &err);
            if (lrc != RG_OK) return rg_set_err(c, lrc == kFlacNotHere ? RG_ERR_FORMAT : lrc, "%s", err.c_str());
        }
        std::vector<rg_track_desc> d;
        std::vector<FlacCounts> counts;
        size_t bytes = 0;
        const int rc = stage_loaded(c, pool, n, &d, &bytes, &counts);
        if (rc != RG_OK) return rc;
        *arena_bytes = bytes;
        for (size_t i = 0; i < n; ++i) {
            descs[i] = d[i];
            infos[i].frames = d[i].frames;
            infos[i].audio_frames = counts[i].decoded;
            infos[i].dropped_frames = counts[i].dropped;
        }
        if (bytes > arena_capacity) return rg_set_err(c, RG_ERR_INVALID_ARG, "arena capacity %zu < %zu bytes", arena_capacity, bytes);
        if (bytes) RG_HIP(c, hipMemcpy(arena_out, c->d_arena.p, bytes, hipMemcpyDeviceToHost));
        return RG_OK;
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}
