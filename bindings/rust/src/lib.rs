//! mp3rgain_amd -- Rust binding of `libmp3rgain_amd.so`, the MI355X-native ReplayGain 1.0 analysis path.
//!
//! **This file cannot be compiled where it is developed** (the build image has neither `rustc` nor `cargo`).  It is kept
//! honest by `tests/test_rust_binding_layout.py`, which parses this file and the C headers and compares every `extern "C"`
//! declaration (name, arity, argument and return types) and every `#[repr(C)]` struct (field order, names, widths,
//! offsets, size -- against a C program compiled from the headers).
//!
//! Two layers:
//! * [`ffi`]: the C ABI of `include/mp3rgain_amd.h` and `include/mp3rgain_amd_node.h`, nothing else.
//! * [`replaygain`]: the names and signatures of mp3rgain's `src/replaygain.rs` -- `analyze_track[_with_index]`
//!   (`:929-941`), `analyze_album[_with_index]` (`:1033-1074`), `find_peak_amplitude` (`:1140`), `is_available`
//!   (`:1119`), the result structs (`:57-95`, `:1125-1132`) -- implemented over the library: a maintainer replaces
//!   `mod replaygain;` by `pub use mp3rgain_amd::replaygain;` and the callers in `src/main.rs` / `src/lib.rs` compile
//!   unchanged.  MPEG Layer III and native FLAC are decoded by the library (on the GPU), WAV is read directly; an M4A/AAC file needs
//!   [`replaygain::set_decoder_command`].
//!
//! The seam *after* the decoder (the host keeps symphonia and hands decoded PCM over) is
//! [`replaygain::analyze_tracks_pcm`] / [`replaygain::analyze_album_pcm`].

#![allow(non_snake_case)]

pub mod ffi {
    //! `extern "C"` declarations; one line per prototype of the headers, in the headers' order.
    use std::os::raw::{c_char, c_int, c_void};

    pub const RG_ABI_VERSION: c_int = 5;
    pub const RG_HISTOGRAM_SIZE: usize = 12000;
    pub const RG_OK: c_int = 0;
    pub const RG_ERR_INVALID_ARG: c_int = -1;
    pub const RG_ERR_UNSUPPORTED_RATE: c_int = -2;
    pub const RG_ERR_DEVICE: c_int = -3;
    pub const RG_ERR_NO_DEVICE: c_int = -4;
    pub const RG_ERR_NOMEM: c_int = -5;
    pub const RG_ERR_STATE: c_int = -6;
    pub const RG_ERR_COLLECTIVE: c_int = -7;
    pub const RG_ERR_IO: c_int = -8;
    pub const RG_ERR_FORMAT: c_int = -9;
    pub const RG_ERR_REFUSED: c_int = -10;
    pub const RG_FMT_F32_PLANAR: u16 = 0;
    pub const RG_FMT_S16_PLANAR: u16 = 1;
    pub const RG_FMT_S32_PLANAR: u16 = 2;
    pub const RG_FILE_MP3: u32 = 0;
    pub const RG_FILE_AAC: u32 = 1;
    pub const RG_TRACK_FLAG_NONFINITE: u32 = 1;
    pub const RG_TRACK_FLAG_IMPRECISE: u32 = 2;
    pub const RG_NODE_EXCHANGE_HOST: c_int = 0;
    pub const RG_NODE_EXCHANGE_RCCL: c_int = 1;

    /// `rg_ctx` (opaque)
    #[repr(C)]
    pub struct RgCtx {
        _p: [u8; 0],
    }
    /// `rg_node` (opaque)
    #[repr(C)]
    pub struct RgNode {
        _p: [u8; 0],
    }
    /// `rg_node_backend` (a test seam of the node header; only ever passed by pointer here)
    #[repr(C)]
    pub struct RgNodeBackend {
        _p: [u8; 0],
    }

    /// `rg_track_desc`: one decoded track inside a caller-owned planar PCM arena
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct RgTrackDesc {
        pub offset_bytes: u64,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u16,
        pub format: u16,
    }

    /// `rg_track_result`: `ReplayGainResult` (src/replaygain.rs:57-68) + `gain_steps()` (:72-74)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct RgTrackResult {
        pub loudness_db: f64,
        pub gain_db: f64,
        pub peak: f64,
        pub sample_rate: u32,
        pub gain_steps: i32,
        pub windows: u32,
        pub file_type: u32,
        pub flags: u32,
        pub reserved: u32,
    }

    /// `rg_album_result`: `AlbumGainResult` minus the per-track vector (src/replaygain.rs:79-95)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct RgAlbumResult {
        pub album_loudness_db: f64,
        pub album_gain_db: f64,
        pub album_peak: f64,
        pub album_gain_steps: i32,
        pub windows: u32,
    }

    /// `rg_peak_result`: `PeakAmplitudeResult` (src/replaygain.rs:1125-1132)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct RgPeakResult {
        pub peak: f64,
        pub peak_pcm: f64,
        pub sample_rate: u32,
        pub reserved: u32,
    }

    /// `rg_device_view`: device-side views for callers that keep results in HBM
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct RgDeviceView {
        pub d_track_hist: *mut c_void,
        pub d_track_result: *mut c_void,
        pub d_album_hist: *mut c_void,
        pub d_album_peak: *mut c_void,
        pub n_tracks: u64,
    }

    /// `rg_wav_info`
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct RgWavInfo {
        pub sample_rate: u32,
        pub channels: u16,
        pub bits_per_sample: u16,
        pub sample_format: u16,
        pub block_align: u16,
        pub reserved: u32,
        pub data_offset: u64,
        pub frames: u64,
    }

    extern "C" {
        // ---- include/mp3rgain_amd.h
        pub fn rg_abi_version() -> c_int;
        pub fn rg_is_available() -> c_int;
        pub fn rg_supported_rate(sample_rate: u32) -> c_int;
        pub fn rg_window_samples(sample_rate: u32) -> u32;
        pub fn rg_hist_loudness(hist: *const u32) -> f64;
        pub fn rg_gain_from_loudness(loudness_db: f64) -> f64;
        pub fn rg_gain_steps(gain_db: f64) -> i32;
        pub fn rg_db_to_steps(db: f64) -> i32;
        pub fn rg_steps_to_db(steps: i32) -> f64;
        pub fn rg_clip_limit_steps(steps: i32, gain_db: f64, peak: f64, prevent_clipping: c_int, wrap_gain: c_int) -> i32;
        pub fn rg_rate_design_info(sample_rate: u32, stable: *mut c_int, halo_frames: *mut u32, decay_ratio: *mut f64) -> c_int;
        pub fn rg_create(device: c_int) -> *mut RgCtx;
        pub fn rg_destroy(ctx: *mut RgCtx);
        pub fn rg_last_error(ctx: *const RgCtx) -> *const c_char;
        pub fn rg_set_stream(ctx: *mut RgCtx, hip_stream: *mut c_void, attach: c_int) -> c_int;
        pub fn rg_wait_user_stream(ctx: *mut RgCtx) -> c_int;
        pub fn rg_batch_stream(ctx: *mut RgCtx) -> *mut c_void;
        pub fn rg_set_kernel(ctx: *mut RgCtx, variant: c_int) -> c_int;
        pub fn rg_set_tuning(ctx: *mut RgCtx, key: c_int, value: i64) -> c_int;
        pub fn rg_tm_design_info(sample_rate: u32, L: u32, H10: *mut u32, rounds: *mut u32, rounds_fast: *mut u32, decoupling_residual: *mut f64, T_out: *mut f64, gram_last_out: *mut f64) -> c_int;
        pub fn rg_tm_design_affine(sample_rate: u32, L: u32, servo: *mut c_int, alpha: *mut f64, beta: *mut f64, g: *mut f64, d_inf: *mut f64, sigma0_out: *mut f64) -> c_int;
        pub fn rg_analyze_pcm_batch(ctx: *mut RgCtx, tracks: *const RgTrackDesc, n: usize, pcm_base: *const c_void, pcm_bytes: usize, pcm_on_device: c_int, out: *mut RgTrackResult, hist_out: *mut u32) -> c_int;
        pub fn rg_analyze_album_pcm(ctx: *mut RgCtx, tracks: *const RgTrackDesc, n: usize, pcm_base: *const c_void, pcm_bytes: usize, pcm_on_device: c_int, tracks_out: *mut RgTrackResult, album_out: *mut RgAlbumResult, album_hist_out: *mut u32) -> c_int;
        pub fn rg_find_peak_pcm(ctx: *mut RgCtx, track: *const RgTrackDesc, pcm_base: *const c_void, pcm_bytes: usize, pcm_on_device: c_int, out: *mut RgPeakResult) -> c_int;
        pub fn rg_enqueue_pcm_batch(ctx: *mut RgCtx, tracks: *const RgTrackDesc, n: usize, d_pcm_base: *const c_void, pcm_bytes: usize, album: c_int) -> c_int;
        pub fn rg_device_view_get(ctx: *mut RgCtx, view: *mut RgDeviceView) -> c_int;
        pub fn rg_collect(ctx: *mut RgCtx, tracks_out: *mut RgTrackResult, hist_out: *mut u32) -> c_int;
        pub fn rg_collect_exact(ctx: *mut RgCtx, tracks: *const RgTrackDesc, n: usize, d_pcm_base: *const c_void, pcm_bytes: usize, tracks_out: *mut RgTrackResult, hist_out: *mut u32) -> c_int;
        pub fn rg_album_allreduce(ctx: *mut RgCtx, nccl_comm: *mut c_void) -> c_int;
        pub fn rg_comm_library(librccl_path: *const c_char) -> c_int;
        pub fn rg_comm_unique_id(id_out: *mut c_void) -> c_int;
        pub fn rg_comm_init(ctx: *mut RgCtx, id: *const c_void, world: c_int, rank: c_int) -> c_int;
        pub fn rg_comm_destroy(ctx: *mut RgCtx) -> c_int;
        pub fn rg_comm_info(ctx: *mut RgCtx, world_out: *mut c_int, version_out: *mut c_int) -> c_int;
        pub fn rg_album_exchange(ctx: *mut RgCtx) -> c_int;
        pub fn rg_album_reduce_gathered(ctx: *mut RgCtx, d_gathered: *const c_void, world: u32) -> c_int;
        pub fn rg_album_finish(ctx: *mut RgCtx, album_out: *mut RgAlbumResult, album_hist_out: *mut u32) -> c_int;
        pub fn rg_album_result_enqueue(ctx: *mut RgCtx) -> c_int;
        pub fn rg_timing_enable(ctx: *mut RgCtx, on: c_int) -> c_int;
        pub fn rg_timing_read(ctx: *mut RgCtx, sum_ms: *mut f64, launches: *mut u64, span_ms: *mut f64, reset: c_int) -> c_int;
        pub fn rg_synth_fill_device(ctx: *mut RgCtx, d_dst_f32: *mut c_void, seed: u64, channel: u32, sample_rate: u32, first_frame: u64, frames: u64) -> c_int;
        pub fn rg_wav_parse(data: *const c_void, len: usize, out: *mut RgWavInfo) -> c_int;
        pub fn rg_set_decoder_command(ctx: *mut RgCtx, command_template: *const c_char) -> c_int;
        pub fn rg_analyze_wav_batch(ctx: *mut RgCtx, wav: *const *const c_void, wav_len: *const usize, n: usize, album: c_int, out: *mut RgTrackResult, album_out: *mut RgAlbumResult) -> c_int;
        pub fn rg_analyze_track(ctx: *mut RgCtx, path: *const c_char, track_index: i32, out: *mut RgTrackResult) -> c_int;
        pub fn rg_analyze_tracks(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, track_index: i32, out: *mut RgTrackResult, status_out: *mut i32) -> c_int;
        pub fn rg_tracks_error(ctx: *const RgCtx, i: usize) -> *const c_char;
        pub fn rg_analyze_album(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, track_index: i32, tracks_out: *mut RgTrackResult, album_out: *mut RgAlbumResult) -> c_int;
        pub fn rg_analyze_album_begin(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, track_index: i32, tracks_out: *mut RgTrackResult, failed_index: *mut usize) -> c_int;
        pub fn rg_analyze_albums(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, album_first: *const usize, n_albums: usize, track_index: i32, tracks_out: *mut RgTrackResult, status_out: *mut i32, albums_out: *mut RgAlbumResult, album_status_out: *mut i32) -> c_int;
        pub fn rg_find_peak_amplitude(ctx: *mut RgCtx, path: *const c_char, out: *mut RgPeakResult) -> c_int;
        pub fn rg_mp3_decode_device(ctx: *mut RgCtx, data: *const c_void, len: usize, ch0: *mut f32, ch1: *mut f32, capacity: u64, info: *mut c_void) -> c_int;
        pub fn rg_mp3_decode_bench(ctx: *mut RgCtx, data: *const c_void, len: usize, copies: u32, reps: u32, ms_out: *mut f64, units_out: *mut u64, compressed_bytes_out: *mut u64, frames_out: *mut u64) -> c_int;
        // ---- include/mp3rgain_amd_node.h
        pub fn rg_node_create(devices: *const c_int, n: usize) -> *mut RgNode;
        pub fn rg_node_destroy(node: *mut RgNode);
        pub fn rg_node_last_error(node: *const RgNode) -> *const c_char;
        pub fn rg_node_devices(node: *const RgNode) -> usize;
        pub fn rg_node_ctx(node: *mut RgNode, i: usize) -> *mut RgCtx;
        pub fn rg_node_set_exchange(node: *mut RgNode, mode: c_int) -> c_int;
        pub fn rg_node_partition(sizes: *const u64, n: usize, world: usize, owner_out: *mut u32);
        pub fn rg_analyze_album_node(node: *mut RgNode, paths: *const *const c_char, n: usize, track_index: i32, tracks_out: *mut RgTrackResult, album_out: *mut RgAlbumResult) -> c_int;
        pub fn rg_analyze_tracks_node(node: *mut RgNode, paths: *const *const c_char, n: usize, track_index: i32, out: *mut RgTrackResult, status_out: *mut i32) -> c_int;
        pub fn rg_node_tracks_error(node: *const RgNode, i: usize) -> *const c_char;
        pub fn rg_node_last_partition(node: *const RgNode, owner_out: *mut u32, n: usize) -> c_int;
        pub fn rg_analyze_albums_node(node: *mut RgNode, paths: *const *const c_char, n: usize, album_first: *const usize, n_albums: usize, track_index: i32, tracks_out: *mut RgTrackResult, status_out: *mut i32, albums_out: *mut RgAlbumResult, album_status_out: *mut i32) -> c_int;
        pub fn rg_node_create_backend(backend: *const RgNodeBackend, devices: *const c_int, n: usize) -> *mut RgNode;
    }
}

pub mod replaygain {
    //! mp3rgain's `replaygain` module (src/replaygain.rs), same names and signatures, run on the GPUs of the node.
    use super::ffi;
    use anyhow::{anyhow, bail, Result};
    use std::ffi::{CStr, CString};
    use std::os::raw::{c_char, c_void};
    use std::os::unix::ffi::OsStrExt;
    use std::path::Path;
    use std::sync::{Mutex, OnceLock};

    /// GAIN_STEP_DB, src/lib.rs:48
    pub const GAIN_STEP_DB: f64 = 1.5;

    /// src/replaygain.rs:48-53
    #[derive(Debug, Clone, Copy, PartialEq)]
    pub enum AudioFileType {
        Mp3,
        Aac,
    }

    /// src/replaygain.rs:57-68
    #[derive(Debug, Clone)]
    pub struct ReplayGainResult {
        pub loudness_db: f64,
        pub gain_db: f64,
        pub peak: f64,
        pub sample_rate: u32,
        pub file_type: AudioFileType,
    }

    impl ReplayGainResult {
        /// src/replaygain.rs:72-74
        pub fn gain_steps(&self) -> i32 {
            (self.gain_db / GAIN_STEP_DB).round() as i32
        }
    }

    /// src/replaygain.rs:79-88
    #[derive(Debug, Clone)]
    pub struct AlbumGainResult {
        pub tracks: Vec<ReplayGainResult>,
        pub album_loudness_db: f64,
        pub album_gain_db: f64,
        pub album_peak: f64,
    }

    impl AlbumGainResult {
        /// src/replaygain.rs:92-94
        pub fn album_gain_steps(&self) -> i32 {
            (self.album_gain_db / GAIN_STEP_DB).round() as i32
        }
    }

    /// src/replaygain.rs:1125-1132
    #[derive(Debug, Clone)]
    pub struct PeakAmplitudeResult {
        pub peak: f64,
        pub peak_pcm: f64,
        pub sample_rate: u32,
    }

    fn to_result(r: &ffi::RgTrackResult) -> ReplayGainResult {
        ReplayGainResult {
            loudness_db: r.loudness_db,
            gain_db: r.gain_db,
            peak: r.peak,
            sample_rate: r.sample_rate,
            file_type: if r.file_type == ffi::RG_FILE_AAC { AudioFileType::Aac } else { AudioFileType::Mp3 },
        }
    }

    unsafe fn text(p: *const c_char) -> String {
        if p.is_null() {
            String::from("mp3rgain_amd: unknown error")
        } else {
            CStr::from_ptr(p).to_string_lossy().into_owned()
        }
    }

    /// All GPUs of the node behind one handle (`rg_node`, include/mp3rgain_amd_node.h): one context and one host thread
    /// per device inside the library.  Calls are serialised by the mutex of [`node`].
    pub struct Node {
        raw: *mut ffi::RgNode,
    }
    // The library's node serialises nothing itself; this binding only ever touches it under the mutex below.
    unsafe impl Send for Node {}

    impl Node {
        /// `devices`: HIP ordinals; empty = every visible device.
        pub fn new(devices: &[i32]) -> Result<Node> {
            if unsafe { ffi::rg_abi_version() } != ffi::RG_ABI_VERSION {
                bail!("libmp3rgain_amd.so has ABI {}, this binding was written for {}", unsafe { ffi::rg_abi_version() }, ffi::RG_ABI_VERSION);
            }
            let raw = unsafe {
                if devices.is_empty() { ffi::rg_node_create(std::ptr::null(), 0) } else { ffi::rg_node_create(devices.as_ptr(), devices.len()) }
            };
            if raw.is_null() {
                bail!("{}", unsafe { text(ffi::rg_node_last_error(std::ptr::null())) });
            }
            Ok(Node { raw })
        }
        fn error(&self) -> anyhow::Error {
            anyhow!("{}", unsafe { text(ffi::rg_node_last_error(self.raw)) })
        }
        /// The context of device `i`, for `rg_set_tuning` / `rg_set_kernel` / the PCM-level calls.
        pub fn ctx(&self, i: usize) -> *mut ffi::RgCtx {
            unsafe { ffi::rg_node_ctx(self.raw, i) }
        }
        pub fn devices(&self) -> usize {
            unsafe { ffi::rg_node_devices(self.raw) }
        }
    }

    impl Drop for Node {
        fn drop(&mut self) {
            unsafe { ffi::rg_node_destroy(self.raw) }
        }
    }

    static NODE: OnceLock<Mutex<Node>> = OnceLock::new();

    /// The process-wide node, created on first use (`MP3RGAIN_AMD_DEVICES=0,2` restricts it, as for the Python CLI).
    pub fn node() -> Result<&'static Mutex<Node>> {
        if let Some(n) = NODE.get() {
            return Ok(n);
        }
        let devices: Vec<i32> = std::env::var("MP3RGAIN_AMD_DEVICES")
            .ok()
            .map(|s| s.split(',').filter_map(|t| t.trim().parse().ok()).collect())
            .unwrap_or_default();
        let n = Node::new(&devices)?;
        Ok(NODE.get_or_init(|| Mutex::new(n)))
    }

    fn c_paths(files: &[&Path]) -> Result<(Vec<CString>, Vec<*const c_char>)> {
        let owned: Vec<CString> = files
            .iter()
            .map(|p| CString::new(p.as_os_str().as_bytes()).map_err(|_| anyhow!("Failed to open: {}", p.display())))
            .collect::<Result<_>>()?;
        let ptrs = owned.iter().map(|s| s.as_ptr()).collect();
        Ok((owned, ptrs))
    }

    fn index_arg(track_index: Option<u32>) -> i32 {
        track_index.map_or(-1, |i| i as i32)
    }

    /// src/replaygain.rs:1119-1121 -- true when the library answers and a gfx950 device is usable (there is no CPU path)
    pub fn is_available() -> bool {
        unsafe { ffi::rg_is_available() != 0 }
    }

    /// Decoder command for files the library does not decode itself (M4A/AAC): a shell template writing WAV to stdout,
    /// `{}` = the quoted path; applied to every device's context.
    pub fn set_decoder_command(command_template: &str) -> Result<()> {
        let c = CString::new(command_template)?;
        let n = node()?.lock().unwrap();
        for i in 0..n.devices() {
            if unsafe { ffi::rg_set_decoder_command(n.ctx(i), c.as_ptr()) } != ffi::RG_OK {
                bail!("{}", unsafe { text(ffi::rg_last_error(n.ctx(i))) });
            }
        }
        Ok(())
    }

    /// src/replaygain.rs:929-932
    pub fn analyze_track(file_path: &Path) -> Result<ReplayGainResult> {
        analyze_track_with_index(file_path, None)
    }

    /// src/replaygain.rs:935-941
    pub fn analyze_track_with_index(file_path: &Path, track_index: Option<u32>) -> Result<ReplayGainResult> {
        let mut v = analyze_tracks_with_index(&[file_path], track_index)?;
        v.remove(0)
    }

    /// The `-r` loop of src/main.rs:1937-2001 as one call: every file's own `Result`, all files decoded and analysed as
    /// one batch per GPU (replicas only; no exchange).
    pub fn analyze_tracks_with_index(files: &[&Path], track_index: Option<u32>) -> Result<Vec<Result<ReplayGainResult>>> {
        let (_owned, ptrs) = c_paths(files)?;
        let mut out = vec![ffi::RgTrackResult::default(); files.len()];
        let mut status = vec![0i32; files.len()];
        let n = node()?.lock().unwrap();
        let rc = unsafe { ffi::rg_analyze_tracks_node(n.raw, ptrs.as_ptr(), ptrs.len(), index_arg(track_index), out.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != ffi::RG_OK {
            return Err(n.error());
        }
        Ok((0..files.len())
            .map(|i| {
                if status[i] == ffi::RG_OK {
                    Ok(to_result(&out[i]))
                } else {
                    Err(anyhow!("{}", unsafe { text(ffi::rg_node_tracks_error(n.raw, i)) }))
                }
            })
            .collect())
    }

    /// src/replaygain.rs:1033-1036
    pub fn analyze_album(files: &[&Path]) -> Result<AlbumGainResult> {
        analyze_album_with_index(files, None)
    }

    /// src/replaygain.rs:1044-1074: the files are dealt to the node's GPUs by size, the first failing file in input order
    /// is the album's error (`:1055`), the devices' histograms and peaks are folded, results come back in input order.
    pub fn analyze_album_with_index(files: &[&Path], track_index: Option<u32>) -> Result<AlbumGainResult> {
        let (_owned, ptrs) = c_paths(files)?;
        let mut tracks = vec![ffi::RgTrackResult::default(); files.len()];
        let mut album = ffi::RgAlbumResult::default();
        let n = node()?.lock().unwrap();
        let rc = unsafe { ffi::rg_analyze_album_node(n.raw, ptrs.as_ptr(), ptrs.len(), index_arg(track_index), tracks.as_mut_ptr(), &mut album) };
        if rc != ffi::RG_OK {
            return Err(n.error());
        }
        Ok(AlbumGainResult {
            tracks: tracks.iter().map(to_result).collect(),
            album_loudness_db: album.album_loudness_db,
            album_gain_db: album.album_gain_db,
            album_peak: album.album_peak,
        })
    }

    /// `analyze_album` for every album of a library in one call (rg_analyze_albums_node): whole albums are dealt to the
    /// node's GPUs, each album's result or its first failing file's error (`:1055`) comes back in input order.
    pub fn analyze_albums(albums: &[Vec<&Path>]) -> Vec<Result<AlbumGainResult>> {
        let files: Vec<&Path> = albums.iter().flat_map(|a| a.iter().copied()).collect();
        let mut first = vec![0usize];
        for a in albums {
            first.push(first.last().unwrap() + a.len());
        }
        let all_fail = |e: anyhow::Error| -> Vec<Result<AlbumGainResult>> { albums.iter().map(|_| Err(anyhow!("{}", e))).collect() };
        let (_owned, ptrs) = match c_paths(&files) {
            Ok(p) => p,
            Err(e) => return all_fail(e),
        };
        let mut tracks = vec![ffi::RgTrackResult::default(); files.len()];
        let mut status = vec![0i32; files.len()];
        let mut out = vec![ffi::RgAlbumResult::default(); albums.len()];
        let mut album_status = vec![0i32; albums.len()];
        let n = match node() {
            Ok(n) => n.lock().unwrap(),
            Err(e) => return all_fail(e),
        };
        let rc = unsafe {
            ffi::rg_analyze_albums_node(n.raw, ptrs.as_ptr(), ptrs.len(), first.as_ptr(), albums.len(), -1, tracks.as_mut_ptr(),
                                        status.as_mut_ptr(), out.as_mut_ptr(), album_status.as_mut_ptr())
        };
        if rc != ffi::RG_OK {
            return all_fail(n.error());
        }
        (0..albums.len())
            .map(|a| {
                if album_status[a] != ffi::RG_OK {
                    let bad = (first[a]..first[a + 1]).find(|&i| status[i] != ffi::RG_OK).unwrap_or(first[a]);
                    return Err(anyhow!("{}", unsafe { text(ffi::rg_node_tracks_error(n.raw, bad)) }));
                }
                Ok(AlbumGainResult {
                    tracks: tracks[first[a]..first[a + 1]].iter().map(to_result).collect(),
                    album_loudness_db: out[a].album_loudness_db,
                    album_gain_db: out[a].album_gain_db,
                    album_peak: out[a].album_peak,
                })
            })
            .collect()
    }

    /// src/replaygain.rs:1140-1249
    pub fn find_peak_amplitude(file_path: &Path) -> Result<PeakAmplitudeResult> {
        let (_owned, ptrs) = c_paths(&[file_path])?;
        let mut out = ffi::RgPeakResult::default();
        let n = node()?.lock().unwrap();
        let ctx = n.ctx(0);
        if unsafe { ffi::rg_find_peak_amplitude(ctx, ptrs[0], &mut out) } != ffi::RG_OK {
            bail!("{}", unsafe { text(ffi::rg_last_error(ctx)) });
        }
        Ok(PeakAmplitudeResult { peak: out.peak, peak_pcm: out.peak_pcm, sample_rate: out.sample_rate })
    }

    /// One decoded track for the seam after the decoder: what `process_audio_buffer` (src/replaygain.rs:953-1029) sees of
    /// a file -- channel 0, channel 1 if there is one (only these two are read, `:971`), the rate.  f32, normalised.
    pub struct DecodedTrack {
        pub left: Vec<f32>,
        pub right: Option<Vec<f32>>,
        pub sample_rate: u32,
        pub file_type: AudioFileType,
    }

    fn arena_of(decoded: &[DecodedTrack]) -> (Vec<f32>, Vec<ffi::RgTrackDesc>) {
        let mut arena: Vec<f32> = Vec::new();
        let mut descs = Vec::with_capacity(decoded.len());
        for t in decoded {
            descs.push(ffi::RgTrackDesc {
                offset_bytes: (arena.len() * 4) as u64,
                frames: t.left.len() as u64,
                sample_rate: t.sample_rate,
                channels: if t.right.is_some() { 2 } else { 1 },
                format: ffi::RG_FMT_F32_PLANAR,
            });
            arena.extend_from_slice(&t.left);
            if let Some(r) = &t.right {
                arena.extend_from_slice(r);
            }
        }
        (arena, descs)
    }

    /// `analyze_track_internal` from the filters onwards (src/replaygain.rs:866-925) for n decoded tracks, on device 0.
    pub fn analyze_tracks_pcm(decoded: &[DecodedTrack]) -> Result<Vec<ReplayGainResult>> {
        let (arena, descs) = arena_of(decoded);
        let mut out = vec![ffi::RgTrackResult::default(); descs.len()];
        let n = node()?.lock().unwrap();
        let ctx = n.ctx(0);
        let rc = unsafe {
            ffi::rg_analyze_pcm_batch(ctx, descs.as_ptr(), descs.len(), arena.as_ptr() as *const c_void, arena.len() * 4, 0, out.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != ffi::RG_OK {
            bail!("{}", unsafe { text(ffi::rg_last_error(ctx)) });
        }
        Ok(out.iter().zip(decoded).map(|(r, d)| ReplayGainResult { file_type: d.file_type, ..to_result(r) }).collect())
    }

    /// The loop of `analyze_album_with_index` (src/replaygain.rs:1053-1074) over decoded tracks, on device 0.
    pub fn analyze_album_pcm(decoded: &[DecodedTrack]) -> Result<AlbumGainResult> {
        let (arena, descs) = arena_of(decoded);
        let mut tracks = vec![ffi::RgTrackResult::default(); descs.len()];
        let mut album = ffi::RgAlbumResult::default();
        let n = node()?.lock().unwrap();
        let ctx = n.ctx(0);
        let rc = unsafe {
            ffi::rg_analyze_album_pcm(ctx, descs.as_ptr(), descs.len(), arena.as_ptr() as *const c_void, arena.len() * 4, 0, tracks.as_mut_ptr(), &mut album, std::ptr::null_mut())
        };
        if rc != ffi::RG_OK {
            bail!("{}", unsafe { text(ffi::rg_last_error(ctx)) });
        }
        Ok(AlbumGainResult {
            tracks: tracks.iter().zip(decoded).map(|(r, d)| ReplayGainResult { file_type: d.file_type, ..to_result(r) }).collect(),
            album_loudness_db: album.album_loudness_db,
            album_gain_db: album.album_gain_db,
            album_peak: album.album_peak,
        })
    }
}

/// The null test of `include/mp3rgain_amd_compare.h`: how does copy b of a recording relate to the reference copy a?  The copies are
/// lined up to the sample on the GPU (a cross-correlation at every lag within a radius of a coarse hint, which comes from the
/// [`fingerprint`] match or from the caller), one gain is fitted, and what is left is sized per block: identical samples some
/// frames apart, the same master after a gain change and a re-dither, a lossy copy, another recording.  The unit of work is a pair
/// of files.  The definitions are a convention of that header, held to no other null-test tool; `lock_permille` and
/// `requant_millilsb2` are measured on synthetic material (`tests/golden/compare_measured.json`).  A module of its own, as
/// [`stereo`] is.  `tests/test_rust_compare_layout.py` compares these declarations with the header.
pub mod compare {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const CMP_COMPLETE: u32 = 1;
    pub const CMP_IDENTICAL: u32 = 2;
    pub const CMP_SHIFTED: u32 = 4;
    pub const CMP_LENGTHS: u32 = 8;
    pub const CMP_INVERTED: u32 = 16;
    pub const CMP_NONFINITE: u32 = 32;
    pub const CMP_LOCKED: u32 = 64;
    pub const CMP_AT_EDGE: u32 = 128;
    pub const CMP_DRIFT: u32 = 256;
    pub const CMP_SAME_MASTER: u32 = 512;
    pub const CMP_DIFFERS: u32 = 1024;
    pub const CMP_UNRELATED: u32 = 2048;
    pub const CMP_RATE: u32 = 4096;
    pub const CMP_NO_OVERLAP: u32 = 8192;
    pub const CMP_NO_COARSE: u32 = 16384;
    pub const CMP_CHANNELS_DIFFER: u32 = 32768;
    pub const CMP_RAW: u32 = 65536;
    pub const CMP_ALIGN_FINGERPRINT: u32 = 0;
    pub const CMP_ALIGN_HINT: u32 = 1;
    pub const CMP_MAX_CHANNELS: usize = 8;
    pub const CMP_MAX_RADIUS: u32 = 2047;
    pub const CMP_MAX_COARSE_RADIUS: u32 = 2047;
    pub const CMP_MAX_SEGMENTS: u32 = 16;
    pub const CMP_MAX_BLOCK_FRAMES: u32 = 384000;
    pub const CMP_DEFAULT_COARSE_RADIUS: u32 = 512;
    pub const CMP_DEFAULT_RADIUS: u32 = 1024;
    pub const CMP_DEFAULT_SEGMENTS: u32 = 4;
    pub const CMP_DEFAULT_SEGMENT_FRAMES: u32 = 262144;
    pub const CMP_DEFAULT_DRIFT_FRAMES: u32 = 1;
    pub const CMP_DEFAULT_LOCK_PERMILLE: u32 = 606;
    pub const CMP_DEFAULT_REQUANT_MILLILSB2: u32 = 18156;

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_compare_pair`: `a` is the reference copy; `hint` in frames, b[n + hint] is expected beside a[n]
    pub struct RgComparePair {
        pub a: u32,
        pub b: u32,
        pub hint: i64,
    }

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_compare_opts`: `block_frames` 0 = the sample rate, `segment_frames` 0 = the whole overlap; a null pointer means the defaults
    pub struct RgCompareOpts {
        pub align: u32,
        pub coarse_radius: u32,
        pub radius: u32,
        pub segments: u32,
        pub segment_frames: u32,
        pub block_frames: u32,
        pub drift_frames: u32,
        pub lock_permille: u32,
        pub requant_millilsb2: u32,
    }

    impl Default for RgCompareOpts {
        fn default() -> Self {
            RgCompareOpts {
                align: CMP_ALIGN_FINGERPRINT,
                coarse_radius: CMP_DEFAULT_COARSE_RADIUS,
                radius: CMP_DEFAULT_RADIUS,
                segments: CMP_DEFAULT_SEGMENTS,
                segment_frames: CMP_DEFAULT_SEGMENT_FRAMES,
                block_frames: 0,
                drift_frames: CMP_DEFAULT_DRIFT_FRAMES,
                lock_permille: CMP_DEFAULT_LOCK_PERMILLE,
                requant_millilsb2: CMP_DEFAULT_REQUANT_MILLILSB2,
            }
        }
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_compare_block`: one block of the overlap, summed over the channels; `first_diff` all ones = no sample differs
    pub struct RgCompareBlock {
        pub aa: i64,
        pub bb: i64,
        pub ab: i64,
        pub first_diff: u64,
        pub equal: u32,
        pub max_diff: u32,
        pub frames: u32,
        pub reserved: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_compare_result`: b[n + lag] lies beside a[n]; `null_db`, `null_unity_db` and `worst_block_db` may be infinite
    pub struct RgCompareResult {
        pub status: i32,
        pub flags: u32,
        pub a: u32,
        pub b: u32,
        pub frames_a: u64,
        pub frames_b: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format_a: u32,
        pub format_b: u32,
        pub dropped_a: u32,
        pub dropped_b: u32,
        pub block_frames: u32,
        pub radius: u32,
        pub segments: u32,
        pub locked_segments: u32,
        pub polarity: i32,
        pub max_diff: u32,
        pub hint: i64,
        pub lag: i64,
        pub seg_lag_min: i64,
        pub seg_lag_max: i64,
        pub overlap: u64,
        pub a_head: u64,
        pub a_tail: u64,
        pub b_head: u64,
        pub b_tail: u64,
        pub blocks: u32,
        pub differing_blocks: u32,
        pub worst_block: u32,
        pub reserved: u32,
        pub equal: u64,
        pub first_diff: u64,
        pub nonfinite: u64,
        pub aa: i64,
        pub bb: i64,
        pub ab: i64,
        pub lock: f64,
        pub gain_db: f64,
        pub null_unity_db: f64,
        pub null_db: f64,
        pub residual_lsb2: f64,
        pub worst_block_db: f64,
        pub gain_min_db: f64,
        pub gain_max_db: f64,
    }

    extern "C" {
        pub fn rg_compare(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, pairs: *const RgComparePair, n_pairs: usize, opts: *const RgCompareOpts,
                          out: *mut RgCompareResult, blocks_out: *mut RgCompareBlock, blocks_per_pair: usize, lag_sums: *mut i64) -> c_int;
    }
}

/// The click scan of `include/mp3rgain_amd_clicks.h`: are there clicks or glitches in each of these WAV, FLAC or MP3 files?  Every
/// channel is predicted block by block by the FLAC encoder's linear model on the GPU; a sample whose residual stands far above the
/// median residual around it is flagged, flagged samples close together make an event, a narrow event is a click and a wide one a
/// burst.  The definitions are a convention of that header, tried on synthetic material only and held to no other tool; the
/// default `ratio_permille` is measured on synthetic material (`tests/golden/clicks_measured.json`).  A module of its own, as
/// [`stereo`] is.  `tests/test_rust_clicks_layout.py` compares these declarations with the header.
pub mod clicks {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const CK_COMPLETE: u32 = 1;
    pub const CK_SILENT: u32 = 2;
    pub const CK_NONFINITE: u32 = 4;
    pub const CK_CLICKS: u32 = 8;
    pub const CK_BURSTS: u32 = 16;
    pub const CK_TRUNCATED: u32 = 32;
    pub const CK_KIND_CLICK: u32 = 1;
    pub const CK_KIND_BURST: u32 = 2;
    pub const CK_MAX_CHANNELS: usize = 8;
    pub const CK_MAX_ORDER: u32 = 12;
    pub const CK_MAX_EVENTS: u32 = 256;
    pub const CK_DEFAULT_BLOCK: u32 = 1024;
    pub const CK_DEFAULT_ORDER: u32 = 8;
    pub const CK_DEFAULT_RATIO_PERMILLE: u32 = 8371;
    pub const CK_DEFAULT_FLOOR: u32 = 4;
    pub const CK_DEFAULT_GAP: u32 = 16;
    pub const CK_DEFAULT_MAX_WIDTH: u32 = 32;
    pub const CK_DEFAULT_MAX_EVENTS: u32 = 16;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_clicks_opts`: every field is taken as it stands; a null pointer means the defaults
    pub struct RgClicksOpts {
        pub block_samples: u32,
        pub order: u32,
        pub ratio_permille: u32,
        pub floor: u32,
        pub gap: u32,
        pub max_width: u32,
        pub max_events: u32,
    }

    impl Default for RgClicksOpts {
        fn default() -> Self {
            RgClicksOpts {
                block_samples: CK_DEFAULT_BLOCK,
                order: CK_DEFAULT_ORDER,
                ratio_permille: CK_DEFAULT_RATIO_PERMILLE,
                floor: CK_DEFAULT_FLOOR,
                gap: CK_DEFAULT_GAP,
                max_width: CK_DEFAULT_MAX_WIDTH,
                max_events: CK_DEFAULT_MAX_EVENTS,
            }
        }
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_clicks_channel`: `first_click` and `strongest_at` equal the record's `frames` when the channel has no click
    pub struct RgClicksChannel {
        pub flagged: u32,
        pub clicks: u32,
        pub bursts: u32,
        pub widest: u32,
        pub first_click: u32,
        pub strongest_at: u32,
        pub strongest_permille: u32,
        pub fallback_blocks: u32,
        pub median_max: u32,
        pub reserved: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_clicks_event`: `kind` is `CK_KIND_CLICK` or `CK_KIND_BURST`, 0 in an unused record
    pub struct RgClicksEvent {
        pub start: u32,
        pub width: u32,
        pub peak_at: u32,
        pub strength_permille: u32,
        pub channel: u16,
        pub kind: u16,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_clicks_result`: `ch[c]` is channel c; `listed` of `events` are in the file's row of the event list
    pub struct RgClicksResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub block_samples: u32,
        pub order: u32,
        pub ratio_permille: u32,
        pub floor: u32,
        pub gap: u32,
        pub max_width: u32,
        pub max_events: u32,
        pub listed: u32,
        pub nonfinite: u64,
        pub events: u64,
        pub ch: [RgClicksChannel; CK_MAX_CHANNELS],
    }

    extern "C" {
        pub fn rg_clicks(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgClicksOpts, out: *mut RgClicksResult,
                         events: *mut RgClicksEvent) -> c_int;
    }
}

/// The FLAC encoder of `include/mp3rgain_amd_flacenc.h`: WAV files with integer samples and FLAC files are decoded by the route the
/// analysis uses and encoded where their PCM lies on the GPU -- an LPC search at every even order, every candidate's Rice coding
/// sized exactly, mid/side for two channels -- and each stream is decoded again by the device decoder and its MD5 held to the
/// source's before its file is written.  An output that exists is never replaced.  A module of its own, as [`stereo`] is.
/// `tests/test_rust_flacenc_layout.py` compares these declarations with the header.
pub mod flacenc {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const FLAC_ENC_DEFAULT_BLOCK: u32 = 4096;
    pub const FLAC_ENC_DEFAULT_LPC: u32 = 8;
    pub const FLAC_ENC_MAX_LPC: u32 = 12;
    pub const FLAC_ENC_VERIFY: u32 = 1;
    pub const FLAC_ENC_COMPLETE: u32 = 1;
    pub const FLAC_ENC_VERIFIED: u32 = 2;
    pub const FLAC_ENC_WRITTEN: u32 = 4;
    pub const FLAC_ENC_VERIFY_FAILED: u32 = 8;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_flac_encode_options`: `block_size` 0 = the default; a null pointer means block 4096, order 8, verified
    pub struct RgFlacEncodeOptions {
        pub struct_size: u32,
        pub block_size: u32,
        pub max_lpc_order: u32,
        pub flags: u32,
    }

    impl Default for RgFlacEncodeOptions {
        fn default() -> Self {
            RgFlacEncodeOptions {
                struct_size: std::mem::size_of::<RgFlacEncodeOptions>() as u32,
                block_size: FLAC_ENC_DEFAULT_BLOCK,
                max_lpc_order: FLAC_ENC_DEFAULT_LPC,
                flags: FLAC_ENC_VERIFY,
            }
        }
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_flac_encode_result`: `md5_pcm` is what STREAMINFO carries, `md5_decoded` what the verified write's decode gave
    pub struct RgFlacEncodeResult {
        pub status: i32,
        pub flags: u32,
        pub pcm_frames: u64,
        pub flac_frames: u32,
        pub dropped_frames: u32,
        pub sample_rate: u32,
        pub channels: u32,
        pub bits_per_sample: u32,
        pub block_size: u32,
        pub min_frame_bytes: u32,
        pub max_frame_bytes: u32,
        pub pcm_bytes: u64,
        pub stream_bytes: u64,
        pub metadata_bytes: u64,
        pub md5_pcm: [u8; 16],
        pub md5_decoded: [u8; 16],
    }

    extern "C" {
        pub fn rg_flac_encode_files(ctx: *mut RgCtx, in_paths: *const *const c_char, out_paths: *const *const c_char, n: usize,
                                    options: *const RgFlacEncodeOptions, results: *mut RgFlacEncodeResult) -> c_int;
    }
}

/// The stereo image scan of `include/mp3rgain_amd_stereo.h`: how do channels 0 and 1 of each of these WAV, FLAC or MP3 files relate?
/// The exact moments of the two channels per block, how many frames are equal, opposite or zero, and the cross-correlation of the
/// channels at every lag within a radius, all on the GPU and all integer in front of the finish: dual mono, an inverted copy, a
/// lopsided or nearly mono image, a channel delayed by a few samples.  The definitions are a convention of that header, tried on
/// synthetic material only and held to no other tool; `delay_permille` and `phase_permille` are measured on synthetic
/// material (`tests/golden/stereo_measured.json`).  A module of its own, as [`dr`] is.  `tests/test_rust_stereo_layout.py` compares these declarations with the header.
pub mod stereo {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const ST_COMPLETE: u32 = 1;
    pub const ST_SILENT: u32 = 2;
    pub const ST_NONFINITE: u32 = 4;
    pub const ST_DUAL_MONO: u32 = 8;
    pub const ST_INVERTED_COPY: u32 = 16;
    pub const ST_OUT_OF_PHASE: u32 = 32;
    pub const ST_NEAR_MONO: u32 = 64;
    pub const ST_ONE_SIDED: u32 = 128;
    pub const ST_DELAYED: u32 = 256;
    pub const ST_MONO: u32 = 512;
    pub const ST_MORE_CHANNELS: u32 = 1024;
    pub const ST_MAX_CHANNELS: usize = 8;
    pub const ST_MAX_RADIUS: u32 = 255;
    pub const ST_MAX_BLOCK_FRAMES: u32 = 384000;
    pub const ST_DEFAULT_RADIUS: u32 = 64;
    pub const ST_DEFAULT_PHASE_PERMILLE: u32 = 587;
    pub const ST_DEFAULT_DELAY_PERMILLE: u32 = 420;
    pub const ST_DEFAULT_MONO_DB: u32 = 40;
    pub const ST_DEFAULT_BALANCE_DB: u32 = 12;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_stereo_opts`: `block_frames` 0 = the sample rate; every other field is taken as it stands; a null pointer means the defaults
    pub struct RgStereoOpts {
        pub block_frames: u32,
        pub radius: u32,
        pub phase_permille: u32,
        pub delay_permille: u32,
        pub mono_db: u32,
        pub balance_db_limit: u32,
    }

    impl Default for RgStereoOpts {
        fn default() -> Self {
            RgStereoOpts {
                block_frames: 0,
                radius: ST_DEFAULT_RADIUS,
                phase_permille: ST_DEFAULT_PHASE_PERMILLE,
                delay_permille: ST_DEFAULT_DELAY_PERMILLE,
                mono_db: ST_DEFAULT_MONO_DB,
                balance_db_limit: ST_DEFAULT_BALANCE_DB,
            }
        }
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_stereo_result`: a positive `lag` means the right channel is late; `balance_db` and `side_db` may be infinite
    pub struct RgStereoResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub block_frames: u32,
        pub radius: u32,
        pub blocks: u32,
        pub active_blocks: u32,
        pub neg_blocks: u32,
        pub mono_blocks: u32,
        pub lag: i32,
        pub anti_lag: i32,
        pub equal_frames: u64,
        pub opposite_frames: u64,
        pub zero_frames: u64,
        pub nonfinite: u64,
        pub ell: i64,
        pub err: i64,
        pub elr: i64,
        pub lag_sum: i64,
        pub anti_sum: i64,
        pub correlation: f64,
        pub lag_correlation: f64,
        pub anti_correlation: f64,
        pub balance_db: f64,
        pub side_db: f64,
    }

    extern "C" {
        pub fn rg_stereo(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgStereoOpts, out: *mut RgStereoResult,
                         lag_sums: *mut i64) -> c_int;
    }
}

/// Duplicates across sample rates (`include/mp3rgain_amd_resample.h`): is this 96 kHz download that CD track?  Every file is brought
/// to 11025 Hz by a rational polyphase resampler on the GPU, fingerprinted there by stage 1 of [`fingerprint`] and matched by its
/// stage 2, whatever the file's own rate.  The options and the pairs are [`fingerprint`]'s; a zero option means this call's default.
/// The threshold is measured on synthetic material only.  `tests/test_rust_resample_layout.py` compares these declarations with the
/// header.
pub mod resample {
    use super::ffi::RgCtx;
    use super::fingerprint::{RgFingerprintOpts, RgFingerprintPair};
    use std::os::raw::{c_char, c_int};

    pub const RS_SHORT: u32 = 1;
    pub const RS_RATE: u32 = 2;
    pub const RS_RATE_OUT: u32 = 11025;
    pub const RS_MAX_PHASES: u32 = 441;
    pub const RS_MAX_RATIO: u32 = 32;
    pub const RS_MIN_RATE: u32 = 8000;
    pub const RS_HALF_PER_W: u32 = 8;
    pub const RS_MAX_CHANNELS: usize = 8;
    /// `RG_XR_*`: what a zero in the options means here
    pub const XR_BLOCK: u32 = 64;
    pub const XR_PROBES: u32 = 8;
    pub const XR_RADIUS: u32 = 128;
    pub const XR_MAX_BER_PERMILLE: u32 = 303;

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_xrate_result`: `rg_fingerprint_result`'s fields for the file's signal at 11025 Hz, then L, M and the resampled count
    pub struct RgXrateResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub fp_frames: u32,
        pub codes: u32,
        pub nonfinite_frames: u32,
        pub group: u32,
        pub matches: u32,
        pub reserved: u32,
        pub codes_at: u64,
        pub frames_at: u64,
        pub up: u32,
        pub down: u32,
        pub resampled: u32,
        pub reserved2: u32,
        pub y_at: u64,
    }

    extern "C" {
        pub fn rg_same_recording_xrate(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgFingerprintOpts, out: *mut RgXrateResult,
                                       pairs: *mut RgFingerprintPair, max_pairs: usize, n_pairs: *mut usize, codes_out: *mut u32, codes_cap: usize) -> c_int;
    }
}

/// The key scan of `include/mp3rgain_amd_key.h`: in which musical key is each of these WAV, FLAC or MP3 files?  The signal
/// decimated to 5 .. 10 kHz, a chroma row per 512 decimated samples from 60 semitone bands (C2 .. B6, A4 = 440 Hz), the rows summed
/// and matched against the Krumhansl-Kessler profiles of the 12 major and 12 minor keys, all on the GPU and all integer after the
/// rows.  The estimator is a convention of that header, tried on synthetic material only and held to no other key finder; key
/// changes are only flagged (`stable_permille`).  A module of its own, as [`tempo`] is.
/// `tests/test_rust_key_layout.py` compares these declarations with the header.
pub mod key {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const KEY_SHORT: u32 = 1;
    pub const KEY_RATE: u32 = 2;
    pub const KEY_NONFINITE: u32 = 4;
    pub const KEY_COMPLETE: u32 = 8;
    pub const KEY_NONE: u32 = 16;
    pub const KEY_MAX_CHANNELS: usize = 8;
    pub const KEY_FRAME: u32 = 4096;
    pub const KEY_HOP: u32 = 512;
    pub const KEY_BANDS: u32 = 60;
    pub const KEY_CHROMA: u32 = 12;
    pub const KEY_RANGE: u32 = 160;
    pub const KEY_TARGET_RATE: u32 = 5000;
    pub const KEY_MAX_DECIM: u32 = 80;
    pub const KEY_TAPS_PER_DECIM: u32 = 16;
    /// `RG_KEY_SEGMENT`: what a zero in the options means
    pub const KEY_SEGMENT: u32 = 128;
    pub const KEY_MIN_SEGMENT: u32 = 8;
    pub const KEY_MAX_SEGMENT: u32 = 4096;
    pub const KEY_ROW_MAX: u32 = 800;

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_key_opts`: a zero means the default; a null pointer likewise
    pub struct RgKeyOpts {
        pub segment: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_key_result`: `key` = 12 mode + tonic, meaningful without `KEY_SHORT`, `KEY_RATE` and `KEY_NONE` in `flags`
    pub struct RgKeyResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub decim: u32,
        pub decimated: u32,
        pub rows: u32,
        pub silent_rows: u32,
        pub nonfinite_frames: u32,
        pub key: u32,
        pub tonic: u32,
        pub mode: u32,
        pub correlation_permille: u32,
        pub margin_permille: u32,
        pub segments: u32,
        pub stable_permille: u32,
        pub chroma_at: u64,
    }

    extern "C" {
        pub fn rg_key(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgKeyOpts, out: *mut RgKeyResult, chroma_out: *mut u16,
                      chroma_cap: usize) -> c_int;
    }
}

/// The tempo scan of `include/mp3rgain_amd_tempo.h`: how fast is each of these WAV, FLAC or MP3 files?  An onset curve per file (one
/// integer per 512 samples from 32 bands between 60 and 8000 Hz), its windowed autocorrelation and a constant-tempo beat grid, all
/// on the GPU and all integer after the onset curve.  The estimator is a convention of that header, tried on synthetic material
/// only and held to no other BPM tool; the reading lies in `[min_bpm, 2 min_bpm)` by convention, drifting tempo is only flagged
/// (`stable_permille`), and the first beat is coarse.  A module of its own, as [`fingerprint`] is.
/// `tests/test_rust_tempo_layout.py` compares these declarations with the header.
pub mod tempo {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const TEMPO_SHORT: u32 = 1;
    pub const TEMPO_RATE: u32 = 2;
    pub const TEMPO_NONFINITE: u32 = 4;
    pub const TEMPO_COMPLETE: u32 = 8;
    pub const TEMPO_RANGE: u32 = 16;
    pub const TEMPO_NONE: u32 = 32;
    pub const TEMPO_MAX_CHANNELS: usize = 8;
    pub const TEMPO_FRAME: u32 = 4096;
    pub const TEMPO_HOP: u32 = 512;
    pub const TEMPO_BANDS: u32 = 32;
    /// `RG_TEMPO_WINDOW`, `RG_TEMPO_WINDOW_HOP`, `RG_TEMPO_MIN_BPM`: what a zero in the options means
    pub const TEMPO_WINDOW: u32 = 1024;
    pub const TEMPO_WINDOW_HOP: u32 = 256;
    pub const TEMPO_MIN_BPM: u32 = 80;
    pub const TEMPO_MIN_WINDOW: u32 = 32;
    pub const TEMPO_MAX_WINDOW: u32 = 1024;
    pub const TEMPO_MAX_HARMONICS: u32 = 8;
    pub const TEMPO_ONSET_MAX: u32 = 1023;
    /// samples added to the best phase of the beat grid: the median `tools/tempo_refcheck.py` measured
    pub const TEMPO_BEAT_BIAS: u32 = 4120;

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_tempo_opts`: a zero field means its default; a null pointer means all defaults
    pub struct RgTempoOpts {
        pub window: u32,
        pub hop: u32,
        pub min_bpm: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_tempo_result`: `period16 == 0` means no tempo; `bpm_milli` is the reading in thousandths of a BPM
    pub struct RgTempoResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub onsets: u32,
        pub windows: u32,
        pub period16: u32,
        pub harmonics: u32,
        pub bpm_milli: u32,
        pub confidence_permille: u32,
        pub stable_permille: u32,
        pub first_beat: u32,
        pub nonfinite_frames: u32,
        pub band_frames: u32,
        pub onsets_at: u64,
    }

    extern "C" {
        pub fn rg_tempo(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgTempoOpts, out: *mut RgTempoResult, onsets_out: *mut u16,
                        onsets_cap: usize) -> c_int;
    }
}

/// The duplicate finder of `include/mp3rgain_amd_fingerprint.h`: which of these WAV, FLAC or MP3 files are the same recording?  A
/// sub-band-difference fingerprint per file (a 32-bit code per 512 samples) and a match of every pair of files at every lag within
/// a radius, both on the GPU.  The fingerprint is a convention of that header, compatible with no other fingerprint, and its
/// threshold was measured on this project's own synthetic material only; matching across sample rates, rates from 96 kHz up,
/// time-stretched or pitch-shifted copies and excerpts offset by more than the radius are not found.  A module of its own, as
/// [`ancestry`] is.  `tests/test_rust_fingerprint_layout.py` compares these declarations with the header.
pub mod fingerprint {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const FP_SHORT: u32 = 1;
    pub const FP_RATE: u32 = 2;
    pub const FP_NONFINITE: u32 = 4;
    pub const FP_COMPLETE: u32 = 8;
    pub const FP_PAIR_COMPARED: u32 = 1;
    pub const FP_PAIR_MATCH: u32 = 2;
    pub const FP_PAIR_SKIPPED: u32 = 4;
    pub const FP_PAIR_PROBE_J: u32 = 8;
    pub const FP_MAX_CHANNELS: usize = 8;
    pub const FP_FRAME: u32 = 4096;
    pub const FP_HOP: u32 = 512;
    pub const FP_BANDS: u32 = 33;
    /// `RG_FP_BLOCK`, `RG_FP_PROBES`, `RG_FP_RADIUS`, `RG_FP_MAX_BER_PERMILLE`: what a zero in the options means
    pub const FP_BLOCK: u32 = 256;
    pub const FP_PROBES: u32 = 8;
    pub const FP_RADIUS: u32 = 512;
    pub const FP_MAX_BER_PERMILLE: u32 = 316;
    pub const FP_MAX_BLOCK: u32 = 4096;
    pub const FP_MAX_PROBES: u32 = 64;
    pub const FP_MAX_RADIUS: u32 = 2047;

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_fingerprint_opts`: a zero field means its default; a null pointer means all defaults
    pub struct RgFingerprintOpts {
        pub block: u32,
        pub probes: u32,
        pub radius: u32,
        pub max_ber_permille: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_fingerprint_result`
    pub struct RgFingerprintResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub fp_frames: u32,
        pub codes: u32,
        pub nonfinite_frames: u32,
        pub group: u32,
        pub matches: u32,
        pub reserved: u32,
        pub codes_at: u64,
        pub frames_at: u64,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_fingerprint_pair`: a matching pair, files `i < j`; `lag` in codes of 512 samples, of the longer file against the shorter
    pub struct RgFingerprintPair {
        pub i: u32,
        pub j: u32,
        pub errors: u32,
        pub bits: u32,
        pub lag: i32,
        pub flags: u32,
    }

    extern "C" {
        pub fn rg_same_recording(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgFingerprintOpts, out: *mut RgFingerprintResult,
                                 pairs: *mut RgFingerprintPair, max_pairs: usize, n_pairs: *mut usize, codes_out: *mut u32, codes_cap: usize) -> c_int;
    }
}

/// The lossy ancestry scan of `include/mp3rgain_amd_ancestry.h`: is this PCM a decoded MPEG Layer III stream?  Every view of a
/// WAV, FLAC or MP3 file (each channel; mid and side of a stereo file) goes through the MP3 encoder's hybrid filterbank at all
/// 576 alignments, and on the stream's granule grid a large share of the spectral lines falls to zero.  The verdict is a
/// convention of that header, tried on this project's own encoder only and held to no other ancestry checker; finely coded
/// streams, short-block passages, other codecs and audio processed after decoding are not found.  A module of its own, as
/// [`dr`] is.  `tests/test_rust_ancestry_layout.py` compares these declarations with the header.
pub mod ancestry {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const ANC_COMPLETE: u32 = 1;
    pub const ANC_MP3_GRID: u32 = 2;
    pub const ANC_MIDSIDE: u32 = 4;
    pub const ANC_NONFINITE: u32 = 8;
    pub const ANC_SHORT: u32 = 16;
    pub const ANC_SILENT: u32 = 32;
    pub const ANC_MAX_CHANNELS: usize = 8;
    pub const ANC_MAX_VIEWS: usize = 10;
    pub const ANC_ALIGNMENTS: u32 = 576;
    pub const ANC_VIEW_MID: u32 = 8;
    pub const ANC_VIEW_SIDE: u32 = 9;
    pub const ANC_SEGMENTS: u32 = 16;
    pub const ANC_GRANULES: u32 = 32;
    /// `RG_ANC_NO_VIEW`: `best_view` of a record without a flagged view
    pub const ANC_NO_VIEW: u32 = 0xFFFF_FFFF;
    /// `RG_ANC_Z_MIN`, `RG_ANC_ISO_MIN`, `RG_ANC_ACTIVE_FLOOR`: what a zero in the options means
    pub const ANC_Z_MIN: f64 = 19.01;
    pub const ANC_ISO_MIN: f64 = 1.675;
    pub const ANC_ACTIVE_FLOOR: f32 = 0.00462963;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_ancestry_opts`: `segments` 0 = the whole plane as one segment; zeros in the last three mean the defaults; a null pointer means 16 segments of 32 granules
    pub struct RgAncestryOpts {
        pub segments: u32,
        pub granules: u32,
        pub z_min: f64,
        pub iso_min: f64,
        pub active_floor: f32,
        pub reserved: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_ancestry_view`
    pub struct RgAncestryView {
        pub ratio: f64,
        pub second: f64,
        pub p0: f64,
        pub z: f64,
        pub iso: f64,
        pub small: u64,
        pub active: u64,
        pub active_total: u64,
        pub offset: u32,
        pub kind: u32,
        pub flagged: u32,
        pub nonfinite: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_ancestry_result`
    pub struct RgAncestryResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub views: u32,
        pub grid_offset: u32,
        pub segments: u32,
        pub granules: u32,
        pub best_view: u32,
        pub reserved: u32,
        pub z: f64,
        pub iso: f64,
        pub view: [RgAncestryView; 10],
    }

    extern "C" {
        pub fn rg_ancestry(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgAncestryOpts, out: *mut RgAncestryResult) -> c_int;
    }
}

/// The dynamic range (DR) figure of `include/mp3rgain_amd_dr.h`: per channel of every WAV, FLAC or MP3 file the mean square and
/// the peak of every 3-second block, the loudest fifth of the blocks and the second-highest block peak, and from them the DR
/// value.  The definitions follow the published description of the TT DR meter and are a convention of that header, unverified
/// against the TT meter or foobar2000.  A module of its own, as [`spectrum`] is.  `tests/test_rust_dr_layout.py` compares these
/// declarations with the header.
pub mod dr {
    use super::ffi::RgCtx;
    use std::os::raw::{c_char, c_int};

    pub const DR_COMPLETE: u32 = 1;
    pub const DR_SILENT: u32 = 2;
    pub const DR_NONFINITE: u32 = 4;
    pub const DR_SHORT: u32 = 8;
    pub const DR_MAX_CHANNELS: usize = 8;
    pub const DR_TOP_PERMILLE: u32 = 200;
    pub const DR_MAX_BLOCK_FRAMES: u32 = 1152000;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_dr_opts`: `block_frames` 0 = 3 * sample rate, `top_permille` 1 .. 1000; a null pointer means `{0, 200}`
    pub struct RgDrOpts {
        pub block_frames: u32,
        pub top_permille: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_dr_channel`
    pub struct RgDrChannel {
        pub dr: f64,
        pub peak_db: f64,
        pub rms_db: f64,
        pub top_ms: f64,
        pub mean_square: f64,
        pub peak: u32,
        pub peak2: u32,
        pub blocks: u32,
        pub top_blocks: u32,
        pub nonfinite: u32,
        pub reserved: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_dr_result`
    pub struct RgDrResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub block_frames: u32,
        pub dr: i32,
        pub dr_mean: f64,
        pub peak_db: f64,
        pub rms_db: f64,
        pub ch: [RgDrChannel; 8],
    }

    extern "C" {
        pub fn rg_dynamic_range(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgDrOpts, out: *mut RgDrResult) -> c_int;
    }
}

/// The spectral scan of `include/mp3rgain_amd_spectrum.h`: per channel of every WAV, FLAC or MP3 file the long-term power
/// spectrum in 256 bands, the frequency above which there is nothing and the depth of the edge there.  A module of its own:
/// [`ffi`] stays the C ABI of `mp3rgain_amd.h` and `mp3rgain_amd_node.h` alone.  `tests/test_rust_spectrum_layout.py` compares
/// these declarations with the header.
pub mod spectrum {
    use super::ffi::{RgCtx, RgTrackDesc};
    use std::os::raw::{c_char, c_int, c_void};

    pub const SPEC_BANDLIMITED: u32 = 1;
    pub const SPEC_UPSAMPLED: u32 = 2;
    pub const SPEC_SHORT: u32 = 4;
    pub const SPEC_NONFINITE: u32 = 8;
    pub const SPEC_COMPLETE: u32 = 16;
    pub const SPEC_MAX_CHANNELS: usize = 8;
    pub const SPEC_BANDS: usize = 256;

    #[derive(Clone, Copy, Debug)]
    #[repr(C)]
    /// `rg_spectrum_opts`: both greater than 0; a null pointer means `{30.0, 4000.0}`
    pub struct RgSpectrumOpts {
        pub edge_db: f64,
        pub min_cutoff_hz: f64,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_spectrum_channel`
    pub struct RgSpectrumChannel {
        pub cutoff_hz: f64,
        pub edge_db: f64,
        pub analysed_frames: u32,
        pub skipped_frames: u32,
        pub flags: u32,
        pub reserved: u32,
    }

    #[derive(Clone, Copy, Debug, Default)]
    #[repr(C)]
    /// `rg_spectrum_result`
    pub struct RgSpectrumResult {
        pub status: i32,
        pub flags: u32,
        pub frames: u64,
        pub sample_rate: u32,
        pub channels: u32,
        pub format: u32,
        pub dropped_frames: u32,
        pub cutoff_hz: f64,
        pub ch: [RgSpectrumChannel; 8],
    }

    extern "C" {
        pub fn rg_spectrum(ctx: *mut RgCtx, paths: *const *const c_char, n: usize, opts: *const RgSpectrumOpts, out: *mut RgSpectrumResult, bands_out: *mut f64) -> c_int;
        pub fn rg_spectrum_arena(ctx: *mut c_void, route: c_int, n: usize, descs: *const RgTrackDesc, opts: *const RgSpectrumOpts, arena: *const c_void, arena_bytes: usize, out: *mut RgSpectrumResult, bands_out: *mut f64) -> c_int;
        pub fn rg_spectrum_verdict(p: *const f64, analysed_frames: u32, sample_rate: u32, opts: *const RgSpectrumOpts, out: *mut RgSpectrumChannel) -> c_int;
        pub fn rg_spectrum_kernel_shape(frame: *mut u32, hop: *mut u32, bands: *mut u32, frames_per_tile: *mut u32) -> c_int;
        pub fn rg_spectrum_rate(ctx: *mut c_void, n: usize, frames: u64, format: u32, host_tracks: usize, threads: u32, reps: u32, warm_ms: f64, kernel_ms: *mut f64, host_ms: *mut f64, mismatches: *mut usize) -> c_int;
    }

    /// The verdict on a caller's 256 band levels (`rg_spectrum_verdict`); `None` for a sample rate of 0 or an option not above 0.
    pub fn verdict(p: &[f64; 256], analysed_frames: u32, sample_rate: u32, opts: Option<RgSpectrumOpts>) -> Option<RgSpectrumChannel> {
        let mut out = RgSpectrumChannel::default();
        let o = opts.as_ref().map_or(std::ptr::null(), |o| o as *const RgSpectrumOpts);
        let rc = unsafe { rg_spectrum_verdict(p.as_ptr(), analysed_frames, sample_rate, o, &mut out) };
        if rc == 0 {
            Some(out)
        } else {
            None
        }
    }
}
