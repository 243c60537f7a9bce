// rg_file_stage.hip -- the loaded files of a batch (rg_file_load.hip) into the planar analysis arena c->d_arena: WAV streams
// through the de-interleave kernels, host-decoded PCM by copy, split MP3 and FLAC streams through their device decoders;
// what the loader pipeline has decoded already stays where it is.
#include <algorithm>

#include "rg_files.h"

namespace rgf {

// Grow the arena to `need` bytes without losing its first `keep` bytes (PCM that chunks decoded earlier in the call).
// The device is idle when this returns from a growth.
int arena_reserve_keep(rg_ctx *c, size_t need, size_t keep) {
    if (need <= c->d_arena.cap) return RG_OK;
    if (keep == 0 || !c->d_arena.p) {
        RG_HIP(c, c->d_arena.reserve(need));
        return RG_OK;
    }
    RG_HIP(c, hipDeviceSynchronize());
    unsigned char *fresh = nullptr;
    const size_t want = need + need / 2 + 16;
    RG_HIP(c, hipMalloc((void **)&fresh, want));
    hipError_t e = hipMemcpy(fresh, c->d_arena.p, keep, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { (void)hipFree(fresh); RG_HIP(c, e); }
    (void)hipFree(c->d_arena.p);
    c->d_arena.p = fresh;
    c->d_arena.cap = want;
    return RG_OK;
}

// the same for loaded files: WAV items take the de-interleave route, decoded MP3 items are planar f32 already and go
// straight into the arena
int stage_loaded(rg_ctx *c, const std::vector<LoadedAudio> &in, size_t n, std::vector<rg_track_desc> *descs, size_t *arena_bytes,
                 std::vector<FlacCounts> *flac_counts) {
    std::vector<WavItem> items(n);
    if (flac_counts) flac_counts->assign(n ? n : 1, FlacCounts{0, 0});
    // streams the loader pipeline has decoded already sit in [0, keep) of the arena; everything else goes behind them
    size_t keep = 0;
    for (size_t i = 0; i < n; ++i)
        if (in[i].kind == LoadedAudio::Staged) keep = std::max(keep, (size_t)align16(in[i].arena_off + (size_t)in[i].walked_frames * in[i].channels * sizeof(float)));
    size_t src_total = 0, dst_total = keep;
    descs->assign(n ? n : 1, rg_track_desc{});
    for (size_t i = 0; i < n; ++i) {
        rg_track_desc &d = (*descs)[i];
        if (in[i].kind == LoadedAudio::Wav) {
            const int lrc = wav_layout(c, i, in[i].wav.data(), in[i].wav.size(), &items[i], &d, &src_total, &dst_total);
            if (lrc != RG_OK) return lrc;
            continue;
        }
        const bool flac = in[i].kind == LoadedAudio::Flac;
        d.frames = in[i].frames;  // (FLAC: every walked frame (device route) or the host decoder's length; fixed below)
        d.sample_rate = in[i].sample_rate;
        d.channels = (uint16_t)in[i].channels;
        d.format = flac ? flac_format(in[i].flac_bps) : (uint16_t)RG_FMT_F32_PLANAR;
        if (in[i].kind == LoadedAudio::Staged) {
            d.offset_bytes = in[i].arena_off;
            continue;
        }
        d.offset_bytes = dst_total;
        dst_total = align16(dst_total + (size_t)in[i].frames * in[i].channels * (flac ? flac_elem_bytes(in[i].flac_bps) : sizeof(float)));
    }
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    RG_HIP(c, c->d_wav.reserve(src_total ? src_total : 16));
    rc = arena_reserve_keep(c, dst_total ? dst_total : 16, keep);
    if (rc != RG_OK) return rc;
    hipStream_t fs = c->file_stream();
    std::vector<RgMp3SplitItem> split;
    std::vector<RgFlacDevStream> flac;
    std::vector<size_t> flac_of;
    for (size_t i = 0; i < n; ++i) {
        unsigned char *dst = c->d_arena.p + (*descs)[i].offset_bytes;
        if (in[i].kind == LoadedAudio::Staged) continue;
        if (in[i].kind == LoadedAudio::Flac) {
            if (in[i].flac_frames.empty()) {  // the host decoder's PCM (or an empty stream)
                if (!in[i].flac_pcm.empty()) RG_HIP(c, hipMemcpyAsync(dst, in[i].flac_pcm.data(), in[i].flac_pcm.size(), hipMemcpyHostToDevice, fs));
                if (in[i].flac_pcm.empty()) (*descs)[i].frames = 0;
                if (flac_counts) (*flac_counts)[i] = FlacCounts{in[i].flac_decoded, in[i].flac_dropped};
                continue;
            }
            RgFlacDevStream st{};
            st.bytes = in[i].file_bytes.data();
            st.len = in[i].file_bytes.size();
            st.frames = in[i].flac_frames.data();
            st.n_frames = (uint32_t)in[i].flac_frames.size();
            st.channels = in[i].channels;
            st.bps = in[i].flac_bps;
            st.elem_bytes = flac_elem_bytes(in[i].flac_bps);
            st.shift = flac_shift(in[i].flac_bps);
            st.dst = dst;
            flac.push_back(st);
            flac_of.push_back(i);
            continue;
        }
        if (in[i].kind == LoadedAudio::Split) {
            RgMp3SplitItem it{};
            it.is = in[i].is.data();
            it.units = in[i].units.data();
            if (!in[i].recs.empty()) {
                it.recs = in[i].recs.data();
                it.main = in[i].main_stream.data();
                it.main_len = in[i].main_stream.size();
            }
            it.n_units = in[i].n_units;
            it.channels = in[i].channels;
            it.rate_row = (uint32_t)rg_mp3_rate_row(in[i].sample_rate);
            it.lsf = in[i].lsf;
            it.d_ch0 = reinterpret_cast<float *>(dst);
            it.d_ch1 = in[i].channels == 2 ? it.d_ch0 + in[i].frames : nullptr;
            split.push_back(it);
            continue;
        }
        if (in[i].kind == LoadedAudio::Planar) {
            const size_t bytes = (size_t)in[i].frames * in[i].channels * sizeof(float);
            if (bytes) RG_HIP(c, hipMemcpyAsync(dst, in[i].planar.data(), bytes, hipMemcpyHostToDevice, fs));
            continue;
        }
        rc = wav_copy_launch(c, items[i], dst, fs);
        if (rc != RG_OK) return rc;
    }
    if (!split.empty()) {  // the device half of the MP3 decoder writes PCM straight into the arena
        rc = rg_mp3dev_decode(c, split.data(), split.size(), fs);
        if (rc != RG_OK) return rc;
    }
    if (!flac.empty()) {  // the device FLAC decoder writes PCM straight into the arena; the decoded lengths come back
        rc = rg_flacdev_decode(c, flac.data(), flac.size(), fs);
        if (rc != RG_OK) return rc;
        for (size_t k = 0; k < flac.size(); ++k) {
            (*descs)[flac_of[k]].frames = flac[k].samples;
            if (flac_counts) (*flac_counts)[flac_of[k]] = FlacCounts{flac[k].decoded_frames, flac[k].dropped_frames};
        }
    }
    // the host buffers are the caller's locals: the copies must have left them before this returns
    RG_HIP(c, hipStreamSynchronize(fs));
    if (!c->user_attached) RG_HIP(c, hipEventRecord(c->user_ev, fs));
    c->user_dirty = true;
    *arena_bytes = dst_total;
    return RG_OK;
}

}  // namespace rgf
