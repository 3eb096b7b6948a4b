/*
 * gypsum_hip.h -- C ABI of libgypsum_hip.so, the MI355X (gfx950) GPS L1 C/A correlator engine.
 *
 * The reference (codyd51/gypsum) is pure Python + numpy and has no FFI layer; its correlator hot path is
 * reached through plain Python call sites.  Each entry point below names the
 * reference interface it replaces (file:line under /root/reference/gypsum).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types cross the boundary.
 *   - return 0 (GYP_OK) or a negative GYP_E_* code; gyp_last_error() gives the message.
 *   - IQ is the reference's on-disk format: interleaved float32 I,Q (antenna_sample_provider.py:112-119),
 *     i.e. complex64.  A "sample" is one I,Q pair.
 *   - functions without a suffix take HOST buffers the caller owns for the duration of the call and are
 *     synchronous.  Functions ending in _dev take DEVICE pointers (allocated with gyp_malloc or by any other
 *     HIP allocator in the same process, e.g. a torch tensor's data_ptr()), are enqueued on the context's
 *     stream and return without synchronising; call gyp_sync() before reading results.
 *   - one context per GPU, not thread-safe (the reference is single-threaded).
 *   - satellite ids are 1..32 everywhere.
 *   - no CPU fallback exists: without a usable HIP device gyp_create fails with GYP_E_NO_DEVICE.
 */
#ifndef GYPSUM_HIP_H
#define GYPSUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): weak-signal
 *      measurement, the fractional code phase and the C/N0 of a weak candidate between the hand-over and the weak bank on the device:
 *      gyp_weak_measure_params(_default), gyp_weak_measured, gyp_weak_measure_fold, gyp_weak_measure(_dev), gyp_weak_measure_estimate,
 *      gyp_weak_measured_state.  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): weak-signal
 *      hand-over, a sub-Hz Doppler refinement between the weak search and the weak bank on the device: gyp_weak_refine_params(_default),
 *      gyp_weak_refined, gyp_weak_refine(_dev), gyp_weak_refine_estimate.  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): weak-signal
 *      tracking, a second kind of channel bank with 20-ms coherent loops and bit synchronisation on the device: gyp_weak_bank,
 *      gyp_weak_params(_default), gyp_weak_ms_rec, gyp_weak_period_rec, gyp_weak_state, gyp_weak_bit_sync, gyp_weak_bank_create / _destroy /
 *      _size / _set_channel / _drop_channel / _get_state / _set_state, gyp_weak_track_block(_dev).  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): weak-signal
 *      acquisition, a hybrid coherent/non-coherent search on the device: gyp_hybrid_cell, gyp_weak_result, GYP_HYB_ALTERNATE,
 *      GYP_HYB_CODE_DOPPLER, gyp_hybrid_stats, gyp_hybrid_shift, gyp_correlate_grid_hybrid(_dev), gyp_acquire_weak(_dev); gyp_debug_set
 *      name hybrid_scratch_mb and the read-only "last_hybrid_chunks".  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): narrowband and
 *      swept interference that is no pure tone, excised in short overlapped transforms on the device: gyp_excisor, GYP_EXCISE_FRAME,
 *      gyp_excise_iq_dev, gyp_iq_spectrum_hist_dev, gyp_excise_from_hist, gyp_ingest_set_excisor, gyp_ingest_get_excisor,
 *      gyp_ingest_find_excisor, gyp_ingest_last_excised.  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): pulsed (wideband)
 *      interference on the device: gyp_blanker, GYP_POWER_HIST_BINS, gyp_blank_iq_dev, gyp_iq_power_hist_dev, gyp_blank_from_hist,
 *      gyp_ingest_set_blanker, gyp_ingest_get_blanker, gyp_ingest_find_pulses, gyp_ingest_last_blanked.  Opt-in.
 * 209 (additions; the number stays): gyp_debug_get's read-only "last_acq_lanes", "last_acq_levels", "last_acq_shared_levels" (what the last
 *      search ran).  gyp_acquire_dev and gyp_search_level_dev refuse, with GYP_E_BAD_ARG, a search of more than 65535 ms or of more than
 *      2^31 - 1 cells (28 per stream and satellite) before anything runs; such a search never worked.
 * 209 (addition; the number stays): gyp_debug_get's read-only "last_track_flow" (what the last gyp_track_block(_dev) call ran).
 * 209 (addition; the number stays): gyp_debug_set name track_finish_all (A/B: the throughput tracking kernel's all-wavefront finish).
 * 209 (additions, as below): signal quality per tracked channel on the device: gyp_quality_sums, gyp_quality, gyp_track_quality_dev,
 *      gyp_track_quality, gyp_quality_from_sums.  Opt-in.
 * 209 (additions; the number stays, nothing that existed changes and a binding looks the new symbols up by name): narrowband
 *      interference on the device: gyp_tone_rec, gyp_notch_tones, gyp_iq_tones_dev, gyp_notch_iq_dev, gyp_tones_find, gyp_tone_refine,
 *      gyp_ingest_set_notches, gyp_ingest_get_notches, gyp_ingest_find_tones; gyp_debug_set name notch_no_lds.  Opt-in.
 * 209: signal conditioning on the device: gyp_iq_stats, gyp_iq_level, gyp_iq_stats_dev, gyp_condition_iq_dev, gyp_iq_level_from_stats,
 *      gyp_ingest_set_level, gyp_ingest_get_level, gyp_ingest_calibrate.  Opt-in: nothing that existed changes.
 * 208: gyp_debug_set / gyp_debug_get name exact_prefetch removed (the software-prefetched form of dll_exact_wave_kernel it selected was
 *      measured slower and is gone); the name is refused like any unknown one.  Nothing else changes.
 * 207: gyp_debug_disc_read added (the float64 discriminators of a bank's last throughput block); gyp_debug_set name no_exact_shared and
 *      the read-only "last_exact_path".  Nothing that existed changes.
 * 206: recordings of 1-, 2- or 4-bit words packed into bytes, unpacked on the device: gyp_packing, gyp_packed_span,
 *      gyp_unpack_iq_dev, gyp_resample_packed_dev, gyp_ingest_open_packed.  Nothing that existed changes.
 * 205: digital down-converter for real-sampled recordings at an intermediate frequency: gyp_ddc_design, gyp_ddc_iq_dev,
 *      gyp_ingest_open_ddc.  Nothing that existed changes.
 * 204: on-device resampler for recordings at any whole-kHz rate: gyp_resample_design, gyp_resample_iq_dev, gyp_ingest_open_resampled;
 *      gyp_debug_set name resample_tile_samples.  Nothing that existed changes.
 * 203: gyp_debug_spec_layout_for added (sub-block length by rate: ~167 ms at 2.046 Msps, r06), gyp_grid_best_bins_refined_dev added (float64
 *      tie-break of the flat grids' best-bin selection); new gyp_debug_set names (no_grid_fused, grid_fused_waves, spec_sub_ms,
 *      widen_wg_per_cu) and the read-only "last_grid_path" / "last_grid_refined_rows"; defaults changed at the end of r06 (same results):
 *      track_chunk_ms 500 -> 250, the widen kernel's grid 8 -> 2 workgroups per CU.
 * 202: gyp_memcpy_d2h_async added (per-ms records leave the device on a copy stream while the next block is tracked).
 * 201: gyp_debug_set / gyp_debug_get / gyp_debug_spec_redo_read / gyp_debug_spec_layout added (the library no longer reads GYP_* environment switches).
 * 200: gyp_chan_out carries the float64 early/late pair (80 bytes), gyp_track_rec::path_info, gyp_debug_track_profile writes
 * 16 values, gyp_params grew; a binding written against another value must not load the library (gypsum_amd/_lib.py checks). */
#define GYP_VERSION 209 /* 0.2.9 */

enum {
    GYP_OK = 0,
    GYP_E_BAD_ARG = -1,
    GYP_E_BAD_RATE = -2,    /* fs not a multiple of 1.023 MHz, N != fs/1000, or an unsupported multiple */
    GYP_E_NO_DEVICE = -3,
    GYP_E_HIP = -4,
    GYP_E_NO_FORMAT = -5,   /* gyp_set_stream_format has not been called */
    GYP_E_NOMEM = -6,
    GYP_E_IO = -7,          /* file could not be opened / read */
    GYP_E_COMM = -8         /* RCCL missing or a collective failed */
};

/* utils.py:23-25 IntegrationType */
enum { GYP_COHERENT = 0, GYP_NON_COHERENT = 1 };

typedef struct gyp_ctx gyp_ctx;

/* ---------------------------------------------------------------- context ---------------------------- */
int gyp_version(void);
int gyp_create(int device_ordinal, gyp_ctx** out);
void gyp_destroy(gyp_ctx* ctx);
/* ctx may be NULL: returns the message of the last failed gyp_create on this thread. */
const char* gyp_last_error(const gyp_ctx* ctx);
int gyp_device_name(gyp_ctx* ctx, char* out, int cap);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own. NULL restores it. */
int gyp_set_stream(gyp_ctx* ctx, void* hip_stream);
int gyp_sync(gyp_ctx* ctx);
/* Two contexts on one device = two HIP streams that run side by side (a receiver's satellite scans beside its tracking:
 * receiver.py:151-161 scans every 10 s while the trackers keep running).  gyp_wait_for makes everything enqueued on
 * `ctx` AFTER this call wait for everything enqueued on `other` BEFORE it (hipEventRecord + hipStreamWaitEvent); the host
 * does not block.  Device buffers are valid in every context of the process. */
int gyp_wait_for(gyp_ctx* ctx, gyp_ctx* other);
/* hipEvent pair on the context's stream: the kernels' device time, as bench.py reports it. */
int gyp_timer_start(gyp_ctx* ctx);
int gyp_timer_stop(gyp_ctx* ctx, float* elapsed_ms);

/* The reference's tunables on this path, with its values as defaults.  What is NOT here: the acquisition integration
 * period (config.py:4: the caller passes n_ms = 10 blocks), the detection threshold (config.py:7: left to the caller of
 * gyp_acquire) and the 250-ms lock window (config.py:23: sizes device-resident rings, compile-time). */
typedef struct gyp_params {
    /* acquisition.py:78-89, 163-167: coarse-to-fine Doppler search */
    double acq_initial_spread_hz;      /* 7000 */
    double acq_min_spread_hz;          /* 10: levels run while spread >= this, spread halves per level */
    double acq_bins_per_spread;        /* 10: bins of a level are range(int(c-s), int(c+s), int(s / this)) */
    /* tracker.py:297-303 code loop */
    double dll_gain;                   /* 0.002 */
    double dll_phase_modulus;          /* 2046 (hard-coded upstream whatever the sample rate) */
    /* tracker.py:227-262 Costas loop */
    double pll_bandwidth_locked_hz;    /* 3 */
    double pll_bandwidth_unlocked_hz;  /* 6 */
    /* tracker.py:157-203 is_locked(), config.py:25 */
    double lock_error_variance_max;    /* 900 */
    double lock_i_variance_max;        /* 2 */
    double lock_rotation_max_deg;      /* 6 */
    /* tracker.py:370-387 circularity watchdog */
    double watchdog_period_s;          /* 6 */
    double watchdog_drop_below;        /* 0.2 */
    double watchdog_nudge_below;       /* 0.93 */
    double watchdog_nudge_hz;          /* 5 (the phase nudge is pi/2 as upstream) */
    /* this library's speculative tracker: a millisecond advances on its window maximum if peak^2 >= kappa * (energy of the
     * millisecond's samples).  Speed only in this sense: every such millisecond is verified against its full profile, so
     * the arg-max, pseudosymbols, lock flags and code phase are the same for every kappa.  The float32 VALUES are not
     * bit-identical across kappa: a fast-path millisecond feeds the loop filters the window's direct sum at the peak lag,
     * a transform-path millisecond (and the throughput kernel) the FFT's value -- the two agree to float32 rounding
     * (~1e-7 relative), and so do peak_re/peak_im/error/doppler_hz/carrier_phase downstream.  Two lags whose |c|^2 the
     * float32 transform cannot order (within 4e-6 relative) count as agreement with the window's choice.
     * The value is quoted for 8184 lags (8.184 Msps): the chance that a noise lag beats a peak of kappa x energy is (lags) x exp(-kappa),
     * so the library applies kappa + ln(N / 8184) at N samples per millisecond (20.7 at 16.368 Msps); 0 stays 0.  At 2.046 Msps it
     * applies a further -5 (20 -> 13.6, with sub-blocks of ~167 ms): there a millisecond off the fast path costs five fast ones and a
     * failed verification one short sub-block (r06, measured: 190 x -> 217-245 x real time at a N = 41, sigma = 6 a). */
    double spec_confidence_kappa;      /* 20 */
    /* acquisition.py:200-219: the reference keeps a cache of integrated profiles keyed by (data, Doppler, PRN) but has its
     * lookup switched off (`if False and key in ...`, "to rule it out as a confounding factor"), so it correlates a bin
     * again when a finer level lands on it (every other bin of levels 2, 3, 8 and 10 with its spreads).  The records are
     * pure functions of (data, satellite, bin): re-evaluating them is redundant work, not part of the result contract.
     * 1 (default): reuse the previous level's record of such a bin -- bit-identical results (tests/test_gpu_params.py),
     * about a fifth of the cells of a search are not evaluated twice.  0: correlate every bin of every level again, as the
     * reference does. */
    double acq_reuse_level_records;    /* 1 */
} gyp_params;
void gyp_params_default(gyp_params* out);
/* Takes effect for calls made afterwards (banks included).  GYP_E_BAD_ARG for values the kernels cannot represent
 * (non-positive spreads / gains / bandwidths, a level with more than 28 Doppler bins). */
int gyp_set_params(gyp_ctx* ctx, const gyp_params* params);
int gyp_get_params(gyp_ctx* ctx, gyp_params* out);

/* Stream descriptor -- replaces SampleProviderAttributes (antenna_sample_provider.py:24-28) and the PRN
 * replica construction of receiver.py:45-53 / satellite.py:20-31.  Requires samples_per_ms == fs_hz/1000 and
 * samples_per_ms == K*1023 with K in {1,2,3,4,5,6,8,10,12,16,20,48} (the reference needs an integer
 * multiple of 1.023 MHz; 2x / 8x / 16x are its recording formats, 48x is BASELINE config 5).  Builds the
 * on-device PRN spectrum table (32 satellites) and the FFT twiddle tables. */
int gyp_set_stream_format(gyp_ctx* ctx, int64_t fs_hz, int32_t samples_per_ms);

/* ---------------------------------------------------------------- PRN codes (host only, no GPU needed) -- */
/* gps_ca_prn_codes.py:134-250 generate_replica_prn_signals: 32 x 1023 chips in {0,1}, row-major, SV 1 first.
 * Fails with GYP_E_BAD_ARG if a generated code misses its IS-GPS-200 first-10-chip marker (:190-247). */
int gyp_prn_chips(uint8_t* out_32x1023);
/* The per-satellite frequency-domain replica in the kernel's register/lane layout: conj(FFT2048(periodic
 * +-1 code))/2048 as float re,im [32 regs][64 lanes]; exposed so tests can check it against numpy. */
int gyp_prn_spectrum_lane_layout(int sat_id, float* out_32x64x2);

/* ---------------------------------------------------------------- device memory helpers --------------- */
int gyp_malloc(gyp_ctx* ctx, uint64_t bytes, void** dptr);
int gyp_free(gyp_ctx* ctx, void* dptr);
int gyp_memcpy_h2d(gyp_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes); /* async on the stream */
int gyp_memcpy_d2h(gyp_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes); /* synchronises */
/* The same enqueued on the context's stream without waiting for it (dst_host page-locked, gyp_host_alloc, for the copy to overlap
 * anything): how a receiver takes a block's gyp_track_rec records -- the EmittedPseudosymbol stream of tracker.py:389 and the
 * code phases receiver.py:110-115 reads -- off the device while the next block is being tracked.  The caller orders it against the
 * producer with gyp_wait_for and reads dst_host after gyp_sync of this context. */
int gyp_memcpy_d2h_async(gyp_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);

/* ---------------------------------------------------------------- correlation cells ------------------- */
/* One (stream, satellite, Doppler) cell of the search grid = one call of
 * utils.py:77-108 integrate_correlation_with_doppler_shifted_prn. */
typedef struct gyp_cell_desc {
    int32_t stream;     /* which IQ stream (0-based) */
    int32_t sat_id;     /* 1..32 */
    double doppler_hz;  /* wipe-off frequency; carrier = exp(-1j*tau*f*t), t from the buffer start (utils.py:92-96) */
    int32_t tap_index;  /* sample offset whose (integrated) complex value is returned in tap_re/tap_im; <0: none */
    int32_t reserved;
} gyp_cell_desc;

/* What acquisition.py:180-189 reduces each integrated profile to. strength (utils.py:111-116) is
 * peak / ((sum - n_max*peak) / (N - n_max)), to be evaluated in float64 by the caller (gyp_cell_strength). */
typedef struct gyp_cell {
    float peak;         /* np.max(profile) */
    int32_t argmax;     /* np.argmax(profile): lowest index among equal maxima */
    double sum;         /* sum(profile) */
    int32_t n_max;      /* number of elements equal to the maximum */
    int32_t reserved;
    float tap_re;       /* coherent integration only: sum_i c_i[desc.tap_index]; 0 otherwise */
    float tap_im;
} gyp_cell;

double gyp_cell_strength(const gyp_cell* c, int32_t samples_per_ms);

/* iq_dev: n_streams x n_ms x N samples, stream-major (stream s starts at sample s*stream_stride).
 * cells_dev/out_dev: n_cells records.  profile_out_dev (may be NULL): the whole integrated profile per cell
 * for callers that need it (utils-level drop-in, tracker_visualizer): non-coherent -> n_cells x N float32
 * (sum |c|); coherent -> n_cells x N x 2 float32 (sum c, interleaved re,im). */
int gyp_correlate_cells_dev(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms,
                            const gyp_cell_desc* cells_dev, int32_t n_cells, int32_t integration,
                            gyp_cell* out_dev, float* profile_out_dev);
/* Host-buffer form: copies iq (n_streams*n_ms*N samples, stream stride n_ms*N) and descriptors in, results out. */
int gyp_correlate_cells(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms,
                        const gyp_cell_desc* cells_host, int32_t n_cells, int32_t integration,
                        gyp_cell* out_host, float* profile_out_host);

/* A flat (satellite x Doppler) search grid in which every satellite uses the SAME Doppler bins -- one level of
 * acquisition.py:154-190 get_best_doppler_shift_estimation for many satellites at once, e.g. BASELINE configs 2/4
 * (range(-5000, 5000, 500), 1 ms) and 5 (range(-10000, 10000, 100), 10 ms coherent).  Same results as
 * gyp_correlate_cells on the corresponding cells, but the carrier wipe-off is done once per (stream, bin) instead
 * of once per (stream, satellite, bin).  out: n_streams x n_sats x n_bins records, bins fastest.
 * Coherent: abs(sum_i c_i) reduced (no tap); non-coherent: sum_i abs(c_i). */
int gyp_correlate_grid_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples,
                           int32_t n_ms, const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host,
                           int32_t n_bins, int32_t integration, gyp_cell* out_dev);
int gyp_correlate_grid(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms,
                       const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins,
                       int32_t integration, gyp_cell* out_host);

/* acquisition.py:180-189 get_best_doppler_shift_estimation's selection over the records of a flat grid: for each of
 * the n_rows = n_streams x n_sats rows of n_bins records (the layout gyp_correlate_grid writes) the first bin holding
 * the largest profile maximum.  This 24-byte record per (stream, satellite) is what a multi-GPU search exchanges. */
typedef struct gyp_best_bin {
    int32_t bin;         /* index into the grid's Doppler bins */
    int32_t argmax;      /* sample_offset_of_correlation_peak */
    float peak;
    int32_t reserved;
    double strength;     /* correlation_strength of that bin's profile */
} gyp_best_bin;
int gyp_grid_best_bins_dev(gyp_ctx* ctx, const gyp_cell* cells_dev, int32_t n_rows, int32_t n_bins, gyp_best_bin* out_dev);
/* The same selection with a float64 tie-break (ABI 203): float32 cells cannot always say which of two bins holds the larger maximum (two
 * bins at equal distance from the true Doppler agree to ~1e-6 by construction).  Every bin of a row whose peak is within 2e-5 of the row's
 * maximum is re-evaluated in float64 from the samples, in the time domain, at its own arg-max lag -- the value acquisition.py:180-182
 * compares -- and the first bin holding the largest wins; gyp_best_bin::reserved = 1 in the rows decided that way (about 1 %).  Takes the
 * grid exactly as gyp_correlate_grid_dev took it (same iq / ids / bins / integration) plus the records it wrote.  Synchronises the stream. */
int gyp_grid_best_bins_refined_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                                   const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins,
                                   int32_t integration, const gyp_cell* cells_dev, gyp_best_bin* out_dev);

/* ---------------------------------------------------------------- acquisition ------------------------- */
/* acquisition.py:35-41 SatelliteAcquisitionAttemptResult */
typedef struct gyp_acq_result {
    int32_t stream;
    int32_t sat_id;
    int32_t doppler_hz;      /* doppler_shift (int, a member of one of the search ranges) */
    int32_t code_phase;      /* prn_phase_shift, sample offset of the correlation peak, [0, N) */
    double carrier_phase;    /* carrier_wave_phase_shift = angle(coherent[code_phase]), radians (-pi, pi] */
    double strength;         /* correlation_strength of the best non-coherent profile */
} gyp_acq_result;

/* acquisition.py:70-152 _attempt_acquisition_for_satellite_id for every (stream, satellite): the 10-level
 * coarse-to-fine Doppler search (spread 7000 Hz halving while >= 10, bins range(int(c-s), int(c+s), int(s/10)),
 * non-coherent over the n_ms blocks), then the coherent pass for the carrier phase.  The threshold of
 * acquisition.py:65 is left to the caller.  out: n_streams x n_sats records, stream-major, sat order as given (at most 32
 * satellites per call).  The _dev form only enqueues work (it never waits for the stream); a scan of four or more streams
 * runs as two halves on two HIP streams of the library's own, joined before the call returns control of the context's
 * stream to whatever the caller enqueues next -- same records bit for bit. */
int gyp_acquire_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples,
                    int32_t n_ms, const int32_t* sat_ids_host, int32_t n_sats, gyp_acq_result* out_dev);
int gyp_acquire(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms,
                const int32_t* sat_ids_host, int32_t n_sats, gyp_acq_result* out_host);
/* ONE level of that search -- acquisition.py:154-190 get_best_doppler_shift_estimation(center, spread, ...) -- with the
 * float64 tie-break between near-equal bins the full search applies: doppler_hz / code_phase / strength of the best
 * bin per (stream, satellite); carrier_phase is 0. */
int gyp_search_level_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                         const int32_t* sat_ids_host, int32_t n_sats, double center_hz, double spread_hz, gyp_acq_result* out_dev);
int gyp_search_level(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms, const int32_t* sat_ids_host,
                     int32_t n_sats, double center_hz, double spread_hz, gyp_acq_result* out_host);

/* ---------------------------------------------------------------- weak-signal acquisition ------------- */
/* The search of gyp_acquire (ten 1-ms blocks summed as |c|, accepted at strength > 3) stops at about 38 dB-Hz.  Below that a
 * satellite is found by integrating coherently over coherent_ms = T milliseconds (1..20) and adding the POWER of n_blocks = M such
 * blocks.  For one stream, satellite and Doppler bin f (Hz, any double):
 *   block b (0 <= b < M) covers milliseconds [bT, (b+1)T); C_b[l], l in [0, N), is its coherent profile: exactly what
 *     gyp_correlate_cells_dev(..., GYP_COHERENT, profile_out) writes for the cell when given that block as its whole buffer (the
 *     wipe-off time starts at the block's first sample);
 *   GYP_HYB_CODE_DOPPLER: delta_b = gyp_hybrid_shift(N, T, b, f, flags) = llround((double)(b T N) * f / 1575420000.0) samples, half
 *     away from zero (a positive Doppler shortens the code period: block b peaks at (cp_0 - delta_b) mod N); else delta_b = 0;
 *   P_k[l] = sum over the blocks b of set k, in increasing b, of |C_b[(l - delta_b) mod N]|^2, float32 throughout (re*re, im*im and
 *     their sum each rounded once), so P is aligned to block 0: its peak is at cp_0;
 *   GYP_HYB_ALTERNATE (needs M >= 2): set 0 holds the even blocks, set 1 the odd ones (with T = 10 a data-bit edge every 20 ms can
 *     fall inside the blocks of one parity only); else every block is in set 0;
 *   per set, with "away" = circular lag distance from argmax greater than N / 1023 samples (one chip): peak = max P, argmax its
 *     lowest index; second, second_argmax the same over the lags away (0, -1 if there are none); n_off, sum_off = sum P and
 *     sumsq_off = sum P^2 over the lags away, float64 in a fixed order (hybrid_reduce_kernel);
 *   the record is that of the set with the larger z (gyp_hybrid_stats); set 0 on a tie or when a z is NaN. */
enum { GYP_HYB_ALTERNATE = 1, GYP_HYB_CODE_DOPPLER = 2 };

typedef struct gyp_hybrid_cell {   /* 48 bytes */
    float peak;
    int32_t argmax;
    float second;
    int32_t second_argmax;
    int32_t n_off;
    int32_t set;            /* the reported set: 0, or 1 (odd blocks, GYP_HYB_ALTERNATE only) */
    double sum_off;
    double sumsq_off;
    int32_t blocks_used;    /* blocks in the reported set */
    int32_t reserved;
} gyp_hybrid_cell;

/* Host only, no GPU.  Float64, in exactly this order, one rounding per operation (no contraction):
 *   n = (double)n_off;  mean = sum_off / n;  m2 = sumsq_off / n;  var = m2 - mean mean;  z = ((double)peak - mean) / sqrt(var),
 *   NaN if n_off <= 0 or !(var > 0);  peak_ratio = (double)peak / (double)second (inf when second is 0 and peak is not).
 * Either output pointer may be NULL.  GYP_E_BAD_ARG for a NULL record. */
int gyp_hybrid_stats(const gyp_hybrid_cell* c, double* z_out, double* peak_ratio_out);
/* Host only, no GPU: delta_b as above (0 without GYP_HYB_CODE_DOPPLER).  n = samples per millisecond. */
int gyp_hybrid_shift(int32_t n, int32_t coherent_ms, int32_t block, double doppler_hz, int32_t flags);

/* The flat-grid twin of gyp_correlate_grid_dev: iq_dev holds n_streams x (n_blocks * coherent_ms) x N samples (stream stride
 * given), out is n_streams x n_sats x n_bins records, bins fastest.  The coherent profiles come from the correlation-cell kernel,
 * one block at a time; cells are processed in chunks whose profile + power scratch fits gyp_debug_set "hybrid_scratch_mb" -- the
 * records are the same bits for every budget.  GYP_E_BAD_ARG, before anything runs, for: coherent_ms outside 1..20; n_blocks < 1;
 * n_blocks * coherent_ms > 65535; GYP_HYB_ALTERNATE with n_blocks < 2; unknown flag bits; satellite ids outside 1..32; a Doppler
 * bin that is not finite; NULL pointers or counts < 1; more than 2^31 - 1 cells.  The _dev form waits for the stream once, after
 * uploading the ids and bins (the host arrays may be temporaries), then only enqueues. */
int gyp_correlate_grid_hybrid_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t coherent_ms,
                                  int32_t n_blocks, int32_t flags, const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host,
                                  int32_t n_bins, gyp_hybrid_cell* out_dev);
int gyp_correlate_grid_hybrid(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t coherent_ms, int32_t n_blocks, int32_t flags,
                              const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins,
                              gyp_hybrid_cell* out_host);

/* What the two-level search returns per (stream, satellite); converts field for field into a gyp_chan_init. */
typedef struct gyp_weak_result {   /* 56 bytes */
    int32_t stream;
    int32_t sat_id;
    double doppler_hz;       /* the final bin */
    int32_t code_phase;      /* argmax of its reported set: the code phase at the buffer's first sample, [0, N) */
    int32_t reserved0;
    double carrier_phase;    /* angle(C_0[code_phase]) of the final bin: the phase at the buffer's first sample, radians (-pi, pi] */
    double z;                /* (peak - mean_off) / std_off of the reported set: the detection statistic */
    double peak_ratio;       /* peak / second */
    int32_t set;
    int32_t reserved;
} gyp_weak_result;

/* Two levels over the grid above, for every (stream, satellite); at most 32 satellites per call.
 *   coarse: bins center_hz - spread_hz + i * (500 / T) Hz, i = 0, 1, ... while < center_hz + spread_hz (half-step scalloping loss
 *     sinc(0.25) = -0.9 dB); the best bin per (stream, satellite) is the one with the largest z, the lowest bin on a tie (a NaN z
 *     never wins);
 *   fine: bins best + j * fine_step_hz for the integers j with |j * fine_step_hz| <= 250 / T, chosen the same way; fine_step_hz <= 0
 *     skips the level.
 * The detection threshold on z is left to the caller, as gyp_acquire leaves its own.  out: n_streams x n_sats records, stream-major,
 * satellites in the order given.  Refusals as gyp_correlate_grid_hybrid_dev, and spread_hz <= 0, non-finite center / spread / step,
 * or a level of more than 4096 bins.  The _dev form only enqueues: it never waits for the stream, not between the levels either. */
int gyp_acquire_weak_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t coherent_ms,
                         int32_t n_blocks, int32_t flags, double center_hz, double spread_hz, double fine_step_hz,
                         const int32_t* sat_ids_host, int32_t n_sats, gyp_weak_result* out_dev);
int gyp_acquire_weak(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t coherent_ms, int32_t n_blocks, int32_t flags,
                     double center_hz, double spread_hz, double fine_step_hz, const int32_t* sat_ids_host, int32_t n_sats,
                     gyp_weak_result* out_host);

/* ---------------------------------------------------------------- tracking: one explicit millisecond -- */
/* Numeric core of tracker.py:264-329 _run_prn_code_tracking_loop_iteration for a batch of channels:
 * carrier wipe-off with (doppler, carrier_phase) at time start_time + n/fs, early/late single-lag correlators at
 * code_phase -/+ 1 sample, full prompt correlation against the PRN rolled by code_phase, its argmax and the
 * reductions peak strength needs.  The loop-filter updates stay with the caller (or use gyp_track_block). */
typedef struct gyp_chan_in {
    int32_t stream;
    int32_t sat_id;
    double doppler_hz;       /* current_doppler_shift */
    double carrier_phase;    /* current_carrier_wave_phase_shift, radians */
    int32_t code_phase;      /* current_prn_code_phase_shift (any integer; rolled mod N like np.roll) */
    int32_t reserved;
} gyp_chan_in;

typedef struct gyp_chan_out {
    float early_re, early_im;   /* np.correlate(xw, roll(prn, s-1)) */
    float late_re, late_im;     /* np.correlate(xw, roll(prn, s+1)) */
    float peak_re, peak_im;     /* coherent_prompt_correlation[argmax |.|] */
    float peak_mag;             /* max |prompt| */
    int32_t peak_offset;        /* argmax of |prompt| (index into the profile of the rolled PRN) */
    double sum;                 /* sum |prompt| */
    int32_t n_max;
    int32_t reserved;
    /* The same early / late correlations to float64 accuracy of the lag-to-lag differences: prompt-lag value (float32
     * transform) -/+ the float64 sums over the chip-transition samples that separate neighbouring lags.  Feed THESE
     * to the DLL discriminator (tracker.py:297): int(self.phase) follows the reference's trajectory with them, which
     * the float32 pair above cannot guarantee near an integer boundary. */
    double early64_re, early64_im;
    double late64_re, late64_im;
} gyp_chan_out;

/* iq_dev: n_streams x N samples of the current millisecond (stream stride given); start_time_host[n_streams]:
 * AntennaSampleChunk.start_time per stream.  profile_out_dev (may be NULL): n_chan x N float32 |prompt|. */
int gyp_track_step_dev(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples,
                       const double* start_time_dev, const gyp_chan_in* chans_dev, int32_t n_chan,
                       gyp_chan_out* out_dev, float* profile_out_dev);
int gyp_track_step(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, const double* start_time_host,
                   const gyp_chan_in* chans_host, int32_t n_chan, gyp_chan_out* out_host,
                   float* profile_out_host);

/* ---------------------------------------------------------------- tracking: device-resident loops ----- */
/* A bank of channels whose whole per-millisecond loop state lives on the GPU: tracker.py:206-389
 * GpsSatelliteTracker.process_samples (code loop, Costas loop with the is_locked() bandwidth switch of
 * :157-203, 6-second circularity watchdog of :370-387) advanced for many milliseconds per launch. */
typedef struct gyp_bank gyp_bank;

typedef struct gyp_chan_init {   /* from SatelliteAcquisitionAttemptResult, pipeline.py:56-62 */
    int32_t stream;
    int32_t sat_id;
    double doppler_hz;
    double carrier_phase;
    int32_t code_phase;
    int32_t reserved;
} gyp_chan_init;

/* one record per channel per millisecond: what process_samples appends to the history deques (tracker.py:146-155) */
typedef struct gyp_track_rec {
    float peak_re, peak_im;       /* correlation_peaks_rolling_buffer entry */
    float strength;               /* correlation_peak_strengths_rolling_buffer entry */
    float discriminator;          /* (|E|^2 - |L|^2)/2 */
    double doppler_hz;            /* current_doppler_shift after the update (doppler_shifts entry) */
    double carrier_phase;         /* current_carrier_wave_phase_shift after the update */
    double error;                 /* carrier_wave_phase_errors entry (I*Q) */
    int32_t code_phase;           /* current_prn_code_phase_shift after the update (int(self.phase), pre-wrap) */
    int32_t peak_offset;
    int8_t pseudosymbol;          /* sign(peak.real): -1, +1, 0 (the reference raises KeyError on 0) */
    int8_t locked;                /* is_locked() as evaluated inside the Costas loop this millisecond */
    int8_t status;                /* 0 ok, 1 LostSatelliteLockError raised this ms (circularity < 0.2), 2 already lost */
    int8_t nudged;                /* circularity watchdog adjusted doppler/phase after this ms */
    /* How the millisecond was evaluated (diagnostic; the record's other fields do not depend on it):
     *   bits 0..1  0 = full transform profile; 1 = window maximum (speculative tracker), confirmed by the verify pass;
     *   bits 8..15 window index of the maximum (the window is the 8 lags around the previous peak), speculative tracker only;
     *   bits 16..31 min(65535, peak^2 / sample energy) the confidence test saw, speculative tracker only. */
    int32_t path_info;
} gyp_track_rec;

int gyp_bank_create(gyp_ctx* ctx, const gyp_chan_init* chans_host, int32_t n_chan, gyp_bank** out);
void gyp_bank_destroy(gyp_bank* bank);
int gyp_bank_size(const gyp_bank* bank);
/* (Re)start channel `index` from an acquisition result: fresh loop state, empty histories, not lost -- what building a
 * new GpsSatelliteSignalProcessingPipeline for the satellite does (pipeline.py:56-63).  Synchronises the stream. */
int gyp_bank_set_channel(gyp_bank* bank, int32_t index, const gyp_chan_init* init_host);
/* Stop advancing channel `index` (the receiver dropping a satellite, receiver.py:259-267): later blocks only write
 * status-2 records for it until gyp_bank_set_channel revives the slot.  Synchronises the stream. */
int gyp_bank_drop_channel(gyp_bank* bank, int32_t index);
/* Advance every channel n_ms milliseconds.  iq_dev: n_streams x n_ms x N (stream stride given);
 * start_time_dev: n_ms doubles (shared by all streams): chunk.start_time of each millisecond, in seconds, any values up to one GPS
 * week (they need not be gapless or increasing: the carrier is wiped off at start_time + n/fs and the watchdog runs on their
 * differences; chunk.end_time is not read -- gyp_bits_push_block takes it); rec_out_dev: n_chan x n_ms records (channel-major), may be NULL.
 * The host form returns GYP_E_BAD_ARG when a channel's stream index is >= n_streams; for the _dev form the caller
 * guarantees that iq_dev holds (largest stream index + 1) streams.  Both return GYP_E_BAD_ARG when the context's stream
 * format is no longer the one the bank was created under.
 * gyp_track_rec::code_phase is int(self.phase) (tracker.py:299); should the accumulator leave the int32 range
 * (un-normalised integer recordings: the discriminator is |E|^2 - |L|^2) the record carries that integer modulo N, sign
 * kept -- the same np.roll shift. */
int gyp_track_block_dev(gyp_bank* bank, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms,
                        const double* start_time_dev, gyp_track_rec* rec_out_dev);
int gyp_track_block(gyp_bank* bank, const float* iq_host, int32_t n_streams, int32_t n_ms,
                    const double* start_time_host, gyp_track_rec* rec_out_host);
/* tracker.py:154,308-309 (GpsSatelliteTrackingParameters.non_coherent_correlation_profiles, read by
 * tracker_visualizer.py:394): keep, for every channel of the bank, the non-coherent prompt profile |corr(wiped samples,
 * PRN rolled by the code phase)| of the trailing milliseconds of each gyp_track_block(_dev) call -- the last
 * min(depth, n_ms) of them (the reference's deque holds 250).  depth = 0 switches it off and frees the rows
 * (n_chan * depth * N floats of device memory: meant for a receiver's dozen channels, not for a 1536-channel bank).
 * While it is on the bank runs on the transform kernel, which forms every millisecond's full profile anyway (the
 * speculative tracker does not).  gyp_bank_read_profiles copies one channel's rows, oldest first, to
 * out[n_rows][N] (out may be NULL to query n_rows); rows of milliseconds a lost channel did not process are undefined. */
int gyp_bank_keep_profiles(gyp_bank* bank, int32_t depth);
int gyp_bank_read_profiles(gyp_bank* bank, int32_t channel, float* out, int32_t* n_rows_out);
/* Re-initialise every channel from n_chan device-resident gyp_chan_init records (same semantics as a fresh
 * gyp_bank_create: histories cleared, DLL phase = code_phase).  Enqueued on the stream. */
int gyp_bank_reset_dev(gyp_bank* bank, const gyp_chan_init* inits_dev);
/* Read back the live estimates (GpsSatelliteTrackingParameters.current_*): n_chan entries each. */
int gyp_bank_get_state(gyp_bank* bank, double* doppler_hz, double* carrier_phase, int32_t* code_phase,
                       int32_t* lost);

/* ---------------------------------------------------------------- weak-signal tracking ------------------ */
/* A second kind of channel bank, for what gyp_acquire_weak finds: gyp_bank is the reference's 1-ms loop (arg-max of a prompt
 * profile, a sign-driven Costas loop), and a 1-ms prompt at 30 dB-Hz has 0 dB SNR.  A weak bank correlates three code lags per
 * sample against NCO-driven replicas, finds the data-bit edge itself and then closes its loops once per 20-ms bit.  No FFT.
 *
 * State of a channel, with fs the sample rate, N samples per millisecond, K = N / 1023, all float64 unless said:
 *   u0     carrier phase in cycles, [0, 1), at the first sample of the current period; f the loop frequency (Hz), f_int its
 *          integrator.  Sample k of the period (0 <= k < P N for a period of P milliseconds, k running across its milliseconds) is
 *          multiplied by exp(-2 pi i (u0 + (f / fs) k)): one quotient, one product, one sum, each rounded once, then the library's
 *          float32 sine/cosine of the reduced phase.  At the period's end u0 <- frac(u0 + (f / fs) (P N)), frac(x) = x - floor(x).
 *   c0     code phase, int64 in units of 2^-40 chip, [0, 1023 2^40), at the CENTRE of the period's first sample.  The rate per sample
 *          is r = llround((1023 / N) (1 + f / 1575.42e6) 2^40) (carrier aiding, from the period's f; products left to right).  The
 *          chip of sample k at lag offset o is ((c0 + o + k r) >> 40) mod 1023, an arithmetic shift and a non-negative remainder, in
 *          exact int64 (below 2^61 at 49.104 Msps).  At the period's end c0 <- (c0 + P N r) mod (1023 2^40).
 *   start  from a gyp_chan_init (or, field for field, a gyp_weak_result): f = f_int = doppler_hz; u0 = frac(carrier_phase / (2 pi)), and 0
 *          where that rounds to 1 (a carrier phase a hair below zero);
 *          c0 = llround((0.5 - code_phase) / K 2^40) mod (1023 2^40) -- the half sample is the sample-centre convention: code_phase
 *          is the sample at which chip 0 begins, and sample 0's centre lies half a sample past its start.
 * Correlators.  Each millisecond yields three complex float32 sums minus, prompt, plus at o = -d, 0, +d (d = gyp_weak_params::spacing,
 * 2^-40 chips).  A millisecond's sums are a pure function of its N samples, the period-start state and its position in the period:
 * one 64-lane wavefront takes the millisecond; lane l adds, in increasing i, the products of samples i = l, l + 64, ... (sample times
 * carrier in float32: re = fma(x.re, c.re, -(x.im c.im)), im = fma(x.re, c.im, x.im c.re); then +- that value by the chip), widened, into float64
 * accumulators; the lanes are reduced in float64 by the fixed tree in which lane l takes lane l + 32, 16, 8, 4, 2, 1, and each of the
 * six sums is rounded to float32 once.  No atomics.
 *
 * Phases (gyp_weak_state::phase), m being the absolute millisecond index:
 *   0 SYNC   the first sync_ms milliseconds from the millisecond the channel was (re)started at.  Open loop: every millisecond is a
 *            period of its own (P = 1), f fixed.  The float32 prompts are kept in the bank; with the last one in, the device picks
 *            the bit edge (gyp_weak_bit_sync over the SYNC span) -- no host round trip.
 *   1 WAIT   open loop as in SYNC, until the first millisecond m at or after the end of SYNC with m mod 20 == edge.
 *   2 TRACK  periods of P = 20 milliseconds.  At the end of a period, with minus_j, prompt_j, plus_j its float32 sums widened:
 *            I + iQ, S-, S+ the float64 sums, in order j = 0..19, of prompt, minus, plus; E- = |S-|, E+ = |S+|; wbp the sum in order
 *            of |prompt_j|^2; bit = I >= 0 ? +1 : -1; mu = (I^2 + Q^2) / wbp (0 if wbp is 0): the NBP / WBP ratio of the "signal
 *            quality" section;
 *            PLL  T = 0.02, wn = pll_bw_hz / 0.53, kp = 1.414 wn, ki = wn^2: dphi = atan(Q / I) (0 when I is 0);
 *                 f_int += ki dphi T / (2 pi); f = f_int + kp dphi / (2 pi);
 *            DLL  dd = 0.5 (E+ - E-) / (E+ + E-) (0 when the sum is 0); after the period's advance of c0,
 *                 c0 <- (c0 + llround(4 dll_bw_hz dd T 2^40)) mod (1023 2^40) (a replica running late makes plus larger).
 *   LOST     once 25 periods are complete and the mean of the last 25 mu (summed oldest first, / 25) is below lose_mu the channel
 *            is lost: that period's record has status 1, every later millisecond of the channel a status-2 record (all else zero),
 *            as after gyp_weak_bank_drop_channel, until gyp_weak_bank_set_channel restarts the slot in SYNC at the bank's cursor.
 *            By the NWPR relation of the signal-quality section mu = 2.5 is 19.3 dB-Hz; noise alone gives 1 +- 0.2.
 *
 * Invariance.  Every record is bit for bit the same however the recording is split into calls (through the SYNC -> TRACK switch and
 * in the middle of a period as well) and whatever other channels the bank holds. */
typedef struct gyp_weak_bank gyp_weak_bank;

typedef struct gyp_weak_params {   /* 48 bytes */
    int32_t period_ms;     /* T in milliseconds: 20 (the only value taken: one data bit) */
    int32_t sync_ms;       /* 400; 40..2000 */
    int64_t spacing;       /* d in 2^-40 chips: 2^39 (half a chip); 1 .. 2^40 */
    double pll_bw_hz;      /* 8; (0, 50] */
    double dll_bw_hz;      /* 1; (0, 10] */
    double lose_mu;        /* 2.5; [0, 20] */
    double reserved;       /* 0 */
} gyp_weak_params;
void gyp_weak_params_default(gyp_weak_params* out);

typedef struct gyp_weak_ms_rec {   /* 32 bytes: one per channel per millisecond */
    float minus_re, minus_im, prompt_re, prompt_im, plus_re, plus_im;
    int16_t pos;           /* position in the period: 0..19 in TRACK, 0 otherwise */
    int8_t phase;          /* 0 SYNC, 1 WAIT, 2 TRACK */
    int8_t status;         /* 0 ok, 2 lost or dropped (every other field 0) */
    int32_t reserved;
} gyp_weak_ms_rec;

typedef struct gyp_weak_period_rec {   /* 88 bytes: one per channel per completed 20-ms period */
    int64_t first_ms;      /* absolute index of the period's first millisecond */
    double f, u0;          /* what the period ran with */
    int64_t c0;
    double i, q, mu, dphi, dd;
    int32_t bit;           /* +1 or -1 (the polarity is ambiguous until a preamble is found, as in the reference) */
    int32_t status;        /* 0 ok, 1 the channel was lost at the end of this period */
    double mu_mean;        /* mean of the last 25 mu including this one; 0 before 25 periods are complete */
} gyp_weak_period_rec;

typedef struct gyp_weak_state {   /* 64 bytes */
    double f, f_int, u0;
    int64_t c0;
    int32_t phase;         /* 0 SYNC, 1 WAIT, 2 TRACK */
    int32_t edge;          /* 0..19; -1 while in SYNC */
    int32_t status;        /* 0 ok, 2 lost or dropped */
    int32_t pos;           /* milliseconds of the current TRACK period already in */
    int32_t n_periods;     /* completed since the (re)start */
    int32_t reserved;
    double mu_mean;        /* as in the last period record */
} gyp_weak_state;

/* Host only, no GPU: the bit edge of a SYNC span.  prompts: n_ms interleaved re,im float32 pairs, the prompt of millisecond
 * first_ms + i at i.  For o in 0..19 the groups are the runs of 20 prompts whose head h has h mod 20 == o and that lie whole inside
 * [first_ms, first_ms + n_ms); en[o] is the mean over those groups, taken in increasing h, of |sum of the 20 prompts|^2: float64, the
 * prompts widened first, re and im summed in order, re re + im im, the squares added in order, one division by the group count (0 for
 * an o without a group).  The edge is the largest en, the lowest o on a tie.  Either output may be NULL.  GYP_E_BAD_ARG for NULL
 * prompts, n_ms < 20 or first_ms < 0. */
int gyp_weak_bit_sync(const float* prompts, int32_t n_ms, int64_t first_ms, double* energies_out20, int32_t* offset_out);

/* first_ms: the absolute index of the first millisecond the bank will be given (its cursor).  Refused with GYP_E_BAD_ARG before
 * anything runs: NULL or counts below 1, params out of range (NULL: the defaults), stream < 0, satellite ids outside 1..32, a
 * non-finite Doppler or carrier phase, first_ms < 0. */
int gyp_weak_bank_create(gyp_ctx* ctx, const gyp_chan_init* chans_host, int32_t n_chan, const gyp_weak_params* params, int64_t first_ms,
                         gyp_weak_bank** out);
void gyp_weak_bank_destroy(gyp_weak_bank* bank);
int gyp_weak_bank_size(const gyp_weak_bank* bank);
/* (Re)start slot `index` in SYNC at the bank's cursor / stop it (status-2 records from then on).  Both synchronise the stream. */
int gyp_weak_bank_set_channel(gyp_weak_bank* bank, int32_t index, const gyp_chan_init* init_host);
int gyp_weak_bank_drop_channel(gyp_weak_bank* bank, int32_t index);
/* The live state of all n_chan channels / the full loop state of one channel, which is put in WAIT with the given edge (TRACK begins
 * at the first millisecond m >= cursor with m mod 20 == edge; status 0, no periods complete).  Of `state` gyp_weak_bank_set_state reads
 * f, f_int, u0 (in [0, 1)), c0 (in [0, 1023 2^40)) and edge (0..19).  Both synchronise the stream. */
int gyp_weak_bank_get_state(gyp_weak_bank* bank, gyp_weak_state* out_host, int64_t* cursor_out);
int gyp_weak_bank_set_state(gyp_weak_bank* bank, int32_t index, const gyp_weak_state* state_host);
/* Advance every channel n_ms milliseconds from the cursor.  iq_dev: (largest stream index + 1) streams of n_ms x N samples, stream
 * stride given.  ms_out_dev: n_chan x n_ms records, channel-major; period_out_dev: n_chan x (n_ms / 20 + 1) records, channel-major,
 * of which the first n_periods_out_dev[channel] are written; either may be NULL (n_periods_out_dev may be NULL too).  Enqueues only.
 * GYP_E_BAD_ARG before anything runs: NULL bank or iq, n_ms < 1 or > 65535, first_ms other than the cursor (recordings with gaps are
 * out of scope), a stride below n_ms N, a context whose stream format is no longer the one the bank was created under.  The host form
 * also refuses a channel whose stream index is >= n_streams; its iq holds n_streams x n_ms x N samples. */
int gyp_weak_track_block_dev(gyp_weak_bank* bank, const float* iq_dev, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                             gyp_weak_ms_rec* ms_out_dev, gyp_weak_period_rec* period_out_dev, int32_t* n_periods_out_dev);
int gyp_weak_track_block(gyp_weak_bank* bank, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                         gyp_weak_ms_rec* ms_out_host, gyp_weak_period_rec* period_out_host, int32_t* n_periods_out_host);

/* ---------------------------------------------------------------- weak-signal hand-over ----------------- */
/* Between gyp_acquire_weak and a weak bank.  The search's fine level steps 10 Hz and the bank's loop pulls in from about 5 Hz, so a
 * 30 dB-Hz candidate handed over as it is starts 7-8 Hz off about one time in four and then false-locks.  This step refines each
 * candidate's Doppler to well below 1 Hz from the open-loop prompts of the search's own buffer (or a longer one), and reports the
 * bit edge and the carrier phase it sees on the way.  It changes nothing in the search, the bank or their records.
 *
 * Inputs: one stream buffer of n_ms whole milliseconds (40..2000) whose first millisecond has the absolute index first_ms, and per
 * candidate a gyp_weak_result, of which stream, sat_id, doppler_hz = f0, carrier_phase and code_phase are read.
 *   1 prompts   p_m, m = 0 .. n_ms - 1, float32 pairs: exactly the prompt a weak bank writes in SYNC for millisecond first_ms + m when
 *               it is created from this result at cursor first_ms -- the start rule, the per-millisecond advance of u0 and c0 and the
 *               arithmetic of a millisecond's sums are those of the "weak-signal tracking" section, bit for bit.
 *   2 pre-sum   L = presum_ms, G = n_ms / L rounded down (a tail shorter than L is dropped).  q_g = the sum, in order, of
 *               p_{gL} .. p_{gL+L-1} widened; s_g = q_g^2: re = qr qr - qi qi, im = (2 qr) qi.  Squaring removes the data bits; s_g
 *               rotates at twice the residual Doppler.  Float64 from here on, one rounding per operation, no contraction.
 *   3 bins      J = floor(span_hz / step_hz); for j = -J .. J: Y_j = sum over g, in increasing g, of s_g exp(-2 pi i c) with
 *               c = (2 (j step_hz)) t_g cycles, t_g = (g L + L / 2) / 1000 s, c reduced by rint(c) before the sine and cosine;
 *               P_j = |Y_j|^2.
 *   4 pick      k = arg-max of P, the lowest index on a tie.  d = 0.5 (P[k-1] - P[k+1]) / (P[k-1] - 2 P[k] + P[k+1]), clamped to
 *               +-0.5; d = 0 when k is an end bin or the denominator is not negative.  delta_hz = (k - J + d) step_hz;
 *               doppler_hz = f0 + delta_hz; bin = k.  status = 1 when k is an end bin: the truth may lie outside the span and the
 *               caller should not trust the result.  A row without a positive P (all-zero prompts) has no peak: bin = J,
 *               delta_hz = 0, peak_to_mean NaN, status 1.
 *   5 quality   peak_to_mean = P[k] over the mean of the P_j with |j - k| > ceil(1000 / (n_ms step_hz)), summed in increasing j;
 *               NaN if there is no such bin.  A figure, not a verdict: on the float64 model 30-60 for a 30 dB-Hz satellite over 220 ms
 *               at the right code phase, 5-20 one sample off, 3-5 for an absent one.
 *   6 phase     Y* = sum over g of s_g exp(-2 pi i (2 delta_hz) t_g); carrier_phase = the input's + 0.5 atan2(Im Y*, Re Y*),
 *               wrapped to (-pi, pi]: right modulo pi, which is all a Costas loop needs.
 *   7 bit edge  p'_m = p_m exp(-2 pi i delta_hz (m + 0.5) / 1000), each part rounded to float32 once; en[o] as gyp_weak_bit_sync
 *               takes it over p'; edge = its pick; edge_ratio = the largest en over the second largest.
 * The device and gyp_weak_refine_estimate share this arithmetic (csrc/refine_plan.hpp) but not their sine and cosine: they agree
 * to about 1e-12 in delta_hz and carrier_phase, not bit for bit.  A candidate's record and prompts are the same bits whatever other
 * candidates the call holds and in whatever order. */
typedef struct gyp_weak_refine_params {   /* 24 bytes */
    double span_hz;        /* 20; (0, 100], and below 250 / presum_ms: the squared sequence is sampled at 1000 / presum_ms Hz and carries 2 f */
    double step_hz;        /* 0.5; [0.01, span_hz]; at most 4097 bins */
    int32_t presum_ms;     /* 4; one of 1, 2, 4, 5, 10, 20 */
    int32_t reserved;      /* 0 */
} gyp_weak_refine_params;
void gyp_weak_refine_params_default(gyp_weak_refine_params* out);

/* Converts by field name into a gyp_chan_init, as gyp_weak_result does. */
typedef struct gyp_weak_refined {   /* 64 bytes */
    int32_t stream;
    int32_t sat_id;
    double doppler_hz;       /* f0 + delta_hz */
    int32_t code_phase;      /* the input's, unchanged */
    int32_t edge;            /* 0..19: a bit edge at every millisecond m with m mod 20 == edge */
    double carrier_phase;    /* at the buffer's first sample, radians (-pi, pi], modulo pi */
    double delta_hz;
    double peak_to_mean;
    double edge_ratio;
    int32_t bin;             /* k, 0 .. 2 J */
    int32_t status;          /* 0 ok, 1 the peak is an end bin (or there is none) */
} gyp_weak_refined;

/* iq_dev: n_streams streams of n_ms x N samples, stream stride given.  results_host: n_results candidates, a HOST array (the caller
 * has thresholded z on the host); out_dev: n_results records in the same order; prompts_out_dev: NULL, or n_results x n_ms float32
 * pairs, candidate-major.  params NULL: the defaults.  Refused with GYP_E_BAD_ARG before anything runs: params out of range as
 * commented above; n_ms outside 40..2000 or fewer than 8 groups; first_ms < 0; NULL pointers or counts below 1; a result with
 * stream < 0 or >= n_streams, a satellite id outside 1..32, a non-finite Doppler or carrier phase, or a code phase outside [0, N); a
 * stride below n_ms N.  The _dev form waits for the stream once, after uploading the candidates (the host array may be a
 * temporary), then only enqueues. */
int gyp_weak_refine_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                        const gyp_weak_result* results_host, int32_t n_results, const gyp_weak_refine_params* params,
                        gyp_weak_refined* out_dev, float* prompts_out_dev);
int gyp_weak_refine(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                    const gyp_weak_result* results_host, int32_t n_results, const gyp_weak_refine_params* params,
                    gyp_weak_refined* out_host, float* prompts_out_host);
/* Host only, no GPU: steps 2-7 on given prompts (n_ms interleaved re,im float32 pairs, the prompt of millisecond first_ms + i at i),
 * the twin of gyp_weak_bit_sync.  The input Doppler and carrier phase are taken as 0, so doppler_hz = delta_hz and carrier_phase is
 * the increment; stream, sat_id and code_phase of *out are 0.  GYP_E_BAD_ARG, with *out untouched, for NULL prompts or out, params
 * out of range (NULL: the defaults), n_ms outside 40..2000 or fewer than 8 groups, first_ms < 0. */
int gyp_weak_refine_estimate(const float* prompts, int32_t n_ms, int64_t first_ms, const gyp_weak_refine_params* params, gyp_weak_refined* out);

/* ---------------------------------------------------------------- weak-signal measurement --------------- */
/* Between gyp_weak_refine and a weak bank.  The hand-over leaves the code phase on the sample grid (+-0.25 chip at 2.046 Msps) and
 * gives no signal level.  This step measures, open loop over the same buffer, the code phase to a fraction of a sample with the
 * bank's own early / late replicas and the C/N0 from the bit-wide coherent sums, and hands the bank a full state
 * (gyp_weak_measured_state -> gyp_weak_bank_set_state), so that it needs no SYNC.  It changes nothing in the search, the hand-over,
 * the bank or their records.
 *
 * Inputs: one stream buffer of n_ms whole milliseconds (40..2000) whose first millisecond has the absolute index first_ms, and per
 * candidate a gyp_weak_refined, of which stream, sat_id, doppler_hz = f, carrier_phase, code_phase and edge are read.  d = spacing / 2^40.
 *   1 start     f, u0, c0 exactly as a weak bank starts ("weak-signal tracking", start) from the candidate read as a gyp_chan_init at
 *               cursor first_ms; per millisecond u0 and c0 advance as in SYNC, with r from f.
 *   2 sums      pass p = 1 .. passes: for every millisecond m the float32 sums minus, prompt, plus at o = -d, 0, +d from the pass's c0, by
 *               the arithmetic of a millisecond's sums of the "weak-signal tracking" section: in pass 1 they are bit for bit the SYNC
 *               gyp_weak_ms_rec of a weak bank created from the candidate at cursor first_ms with this spacing; in a later pass the
 *               six sums are those of a bank put at the pass's c0 through gyp_weak_bank_set_state, while it waits.  In the same loop
 *               W_m = sum |x|^2: lane l adds, in increasing i, (re re + im im) of the widened samples i = l, l + 64, ... in float64
 *               (two products, one sum, one addition, each rounded once); the lanes are reduced by the same tree; a float64.
 *   3 fold      the groups are gyp_weak_bit_sync's for o = edge: heads h = first_ms + ((edge - first_ms) mod 20), h + 20, ... with
 *               h + 20 <= first_ms + n_ms; n_groups of them.  Float64 from here on, one rounding per operation, no contraction.
 *               Per group, with S the sum in order of its 20 float32 sums widened (re and im apart): e = S.re S.re + S.im S.im for
 *               each of minus, prompt, plus; w = the sum in order of its 20 W_m.  E-, E0, E+ and Wn are the sums, in increasing h, of
 *               the groups' e and w.  Wn is what white noise alone is expected to leave in each E (|chip| = |carrier| = 1).
 *               A. = sqrt(max(E. - Wn, 0)).
 *   4 correct   dd = (1 - d) (A+ - A-) / (A+ + A-), d = (double)spacing / 2^40; with d = 1/2 the bank's DLL discriminator.  When
 *               A+ + A- is not positive, dd = 0 and status bit 1 is set.  c0 <- (c0 + llround(dd 2^40)) mod (1023 2^40): a replica
 *               running late makes plus larger, as in the bank.  The next pass starts from the corrected c0 with f and u0 unchanged;
 *               the correction stays on the device between passes.
 *   5 record    c0 after the last pass's correction; code_phase_samples = 0.5 - K (c0 / 2^40), + N when negative (and 0 where that
 *               rounds to N): the inverse of the start rule, in [0, N); delta_chips = the sum, in order, of the passes' dd;
 *               dd_last = the last pass's dd: the residual by which the caller judges convergence;
 *               cn0_dbhz = 10 log10(((E0 - Wn) / Wn) / 0.020) of the last pass, NaN when E0 <= Wn or Wn is 0.
 * Figures, not verdicts.  The sample-lattice limit: every supported rate has a whole number of samples per chip, so where the code
 * drifts less than one sample across the buffer (about 0.65 chip/s per kHz of Doppler: below 3.6 kHz over 220 ms at 2.046 Msps) the
 * envelope is a staircase in the code offset, the early-late difference has a dead zone and the error stays near the grid's
 * ("weak-signal measurement").  That is a property of the recording and the bank's DLL has it too.
 * The device and gyp_weak_measure_estimate share this arithmetic (csrc/measure_plan.hpp); + - x / and sqrt are correctly rounded on
 * both, so dd and c0 agree bit for bit on the same sums, cn0_dbhz (the platform's log10) to about 1e-12.  A candidate's record, sums
 * and folds are the same bits whatever other candidates the call holds and in whatever order. */
typedef struct gyp_weak_measure_params {   /* 16 bytes */
    int64_t spacing;       /* d in 2^-40 chips: 2^39 (half a chip); 2^36 .. 2^39 */
    int32_t passes;        /* 2; 1..4 */
    int32_t reserved;      /* 0 */
} gyp_weak_measure_params;
void gyp_weak_measure_params_default(gyp_weak_measure_params* out);

typedef struct gyp_weak_measured {   /* 80 bytes */
    int32_t stream;              /* offset 0 */
    int32_t sat_id;              /* 4 */
    double doppler_hz;           /* 8: the input's */
    double carrier_phase;        /* 16: the input's */
    int64_t c0;                  /* 24: 2^-40 chips at the centre of the buffer's first sample, [0, 1023 2^40) */
    double code_phase_samples;   /* 32: [0, N) */
    double delta_chips;          /* 40 */
    double dd_last;              /* 48 */
    double cn0_dbhz;             /* 56 */
    int32_t edge;                /* 64: the input's */
    int32_t n_groups;            /* 68 */
    int32_t status;              /* 72: 0 ok; bit 1 (value 1): no envelope above the noise in some pass -- c0 is the start plus whatever
                                    corrections were made */
    int32_t reserved;            /* 76 */
} gyp_weak_measured;

/* One pass's fold and correction (steps 3-4). */
typedef struct gyp_weak_measure_fold {   /* 64 bytes */
    double e_minus, e_prompt, e_plus;   /* 0, 8, 16: E-, E0, E+ */
    double wn;                          /* 24 */
    double dd;                          /* 32 */
    double cn0_dbhz;                    /* 40: as in the record, of this pass */
    int64_t c0;                         /* 48: after this pass's correction */
    int32_t n_groups;                   /* 56 */
    int32_t status;                     /* 60: 0, or 1 when A+ + A- is not positive */
} gyp_weak_measure_fold;

/* iq_dev: n_streams streams of n_ms x N samples, stream stride given.  refined_host: n_results candidates, a HOST array; out_dev:
 * n_results records in the same order.  Optional outputs, each NULL or candidate-major, pass-major within a candidate:
 * sums_out_dev n_results x passes x n_ms gyp_weak_ms_rec (phase 0, pos 0, status 0), w_out_dev as many
 * float64 W_m, folds_out_dev n_results x passes records.  params NULL: the defaults.  Refused with GYP_E_BAD_ARG before anything runs:
 * spacing outside 2^36 .. 2^39 or passes outside 1..4; n_ms outside 40..2000, or no whole group of 20 milliseconds at a candidate's
 * edge; first_ms < 0; NULL pointers or counts below 1; a candidate with stream < 0 or >= n_streams, a satellite id outside 1..32, a
 * non-finite Doppler or carrier phase, a code phase outside [0, N) or an edge outside 0..19; a stride below n_ms N.  The _dev form
 * waits for the stream once, after uploading the candidates (the host array may be a temporary), then only enqueues: 3 launches a pass. */
int gyp_weak_measure_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                         const gyp_weak_refined* refined_host, int32_t n_results, const gyp_weak_measure_params* params,
                         gyp_weak_measured* out_dev, gyp_weak_ms_rec* sums_out_dev, double* w_out_dev, gyp_weak_measure_fold* folds_out_dev);
int gyp_weak_measure(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                     const gyp_weak_refined* refined_host, int32_t n_results, const gyp_weak_measure_params* params,
                     gyp_weak_measured* out_host, gyp_weak_ms_rec* sums_out_host, double* w_out_host, gyp_weak_measure_fold* folds_out_host);
/* Host only, no GPU: steps 3-4 of one pass on given sums (n_ms records, that of millisecond first_ms + i at i; of each the six sums
 * are read) and w (n_ms float64), from the pass's c0.  GYP_E_BAD_ARG, with *out untouched, for NULL sums, w or out, spacing outside
 * 2^36 .. 2^39, n_ms outside 40..2000, first_ms < 0, edge outside 0..19, no whole group, c0 outside [0, 1023 2^40). */
int gyp_weak_measure_estimate(const gyp_weak_ms_rec* sums, const double* w, int32_t n_ms, int64_t first_ms, int32_t edge, int64_t spacing,
                              int64_t c0, gyp_weak_measure_fold* out);
/* Host only, no GPU: the state gyp_weak_bank_set_state takes, from a record, advanced ms_ahead milliseconds as in SYNC (f = f_int =
 * doppler_hz, u0 by the start rule from carrier_phase, c0 the record's; phase 1, the record's edge, all else 0).  ms_ahead 0: for a
 * bank whose cursor is the buffer's first_ms; n_ms: for one that continues behind the buffer.  fs: samples per second, N: samples
 * per millisecond.  GYP_E_BAD_ARG for NULL, fs < 1, N not a positive multiple of 1023, ms_ahead outside 0..65535, a non-finite
 * Doppler or carrier phase, c0 outside [0, 1023 2^40), edge outside 0..19. */
int gyp_weak_measured_state(const gyp_weak_measured* rec, int64_t fs, int32_t samples_per_ms, int32_t ms_ahead, gyp_weak_state* out);

/* ---------------------------------------------------------------- multi-GPU ----------------------------- */
/* The path shards by stream, satellite or (satellite x Doppler) cell with no data-path exchange except ONE all-gather
 * of fixed-size result records per batch (SURVEY.md 8 e; the reference itself is single-process).  One process per
 * GPU; the communicator is RCCL's (librccl is dlopen'ed on first use -- the copy the process already holds, e.g.
 * torch's, else the system one -- so nothing here is needed, or loaded, on a single GPU).
 *   rank 0: gyp_comm_unique_id(id); every rank receives the 128 bytes by any out-of-band means (MPI, a file, a gloo
 *   broadcast ...) and calls gyp_comm_init(ctx, rank, world, id) with its own context.
 * gyp_comm_init(ctx, 0, 1, NULL) declares a single-process "world" without touching RCCL: gyp_allgather_dev is then a
 * device copy.  With an id and world == 1 a real one-rank RCCL communicator is created. */
#define GYP_COMM_ID_BYTES 128
int gyp_comm_unique_id(void* out_128_bytes);
int gyp_comm_init(gyp_ctx* ctx, int32_t rank, int32_t world, const void* unique_id_128_bytes);
int gyp_comm_destroy(gyp_ctx* ctx);
int gyp_comm_info(gyp_ctx* ctx, int32_t* rank, int32_t* world, int32_t* uses_rccl);
/* recv_dev[r * bytes_per_rank ...] = rank r's send_dev, on every rank.  Enqueued on the context's stream behind the
 * kernels that wrote send_dev (ncclAllGather over xGMI); no host synchronisation.  Records are opaque bytes. */
int gyp_allgather_dev(gyp_ctx* ctx, const void* send_dev, void* recv_dev, uint64_t bytes_per_rank);

/* ---------------------------------------------------------------- host staging ------------------------- */
/* Page-locked host memory for callers that feed IQ from the host (asynchronous gyp_memcpy_h2d needs it). */
int gyp_host_alloc(gyp_ctx* ctx, uint64_t bytes, void** out);
int gyp_host_free(gyp_ctx* ctx, void* p);
/* Integer recordings that crossed PCIe in file width: out_dev[i] = (float)raw_dev[i] * scale for n_words interleaved
 * I,Q words of format GYP_FMT_I8 / GYP_FMT_U8 / GYP_FMT_I16 (see the ingest section), on the context's stream. */
int gyp_widen_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, uint64_t n_words, float scale, float* out_dev);

/* ---------------------------------------------------------------- synthetic IQ (bench / test support) ---- */
/* No recording ships with the reference (vendored_signals/ is git-ignored), so benchmarks run on synthetic
 * baseband generated straight into HBM:  x[n] = sum_k a_k * code_k[(n - cp_k) mod N] * bit_k(n) *
 * exp(1j*(2*pi*d_k*n/fs + phi_k)) + sigma*(N(0,1) + 1j*N(0,1)),  bit_k = +-1 per 20 ms from a counter hash
 * (gyp_synth_nav_bit gives the same value on the host).  Noise is a counter-based hash + Box-Muller keyed by
 * (seed, stream, n). */
typedef struct gyp_synth_sat {
    int32_t sat_id;        /* 1..32 */
    int32_t code_phase;    /* samples, [0, N) */
    double doppler_hz;
    double carrier_phase;  /* radians */
    float amplitude;
    int32_t nav_bit_offset_ms;
} gyp_synth_sat;

/* out_dev: n_streams x n_ms x N samples (stream stride given); sats_host: n_streams x n_sats descriptors. */
int gyp_synth_iq_dev(gyp_ctx* ctx, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     const gyp_synth_sat* sats_host, int32_t n_sats, float noise_sigma, uint64_t seed);
/* +-1 data bit satellite `sat_id` of stream `stream` carries during millisecond `ms` (host mirror of the kernel). */
int gyp_synth_nav_bit(uint64_t seed, int32_t stream, int32_t sat_id, int32_t nav_bit_offset_ms, int64_t ms);

/* ---------------------------------------------------------------- navigation bits (host) -------------- */
/* SURVEY.md 8 f4.  Host-side replacement for gypsum/navigation_bit_intergrator.py:100-288
 * NavigationBitIntegrator: one integrator per tracking channel, fed the 1 kHz pseudosymbols, emitting the
 * 50 bit/s EmitNavigationBitEvent stream with the reference's bit-phase selection / resynchronisation rules.
 * No GPU involved; errors are reported through gyp_last_error(NULL). */
typedef struct gyp_bits gyp_bits;

#define GYP_BIT_ZERO 0      /* tracker.py:48-51 BitValue.ZERO */
#define GYP_BIT_ONE 1       /* BitValue.ONE */
#define GYP_BIT_UNKNOWN 2   /* BitValue.UNKNOWN */

/* navigation_bit_intergrator.py:29-39 EmitNavigationBitEvent */
typedef struct gyp_bit_event {
    double receiver_timestamp;                 /* start_of_pseudosymbol of the bit's first pseudosymbol */
    double trailing_edge_receiver_timestamp;   /* end_of_pseudosymbol of its last pseudosymbol */
    int32_t channel;
    int32_t bit_value;                         /* GYP_BIT_* */
} gyp_bit_event;

/* navigation_bit_intergrator.py:55-74 NavigationBitIntegratorHistory scalars (+ NavigationBitIntegrator.slide) */
typedef struct gyp_bits_state {
    int32_t determined_bit_phase;          /* -1 = None */
    int32_t previous_bit_phase_decision;   /* -1 = None */
    int32_t sequential_unknown_bit_value_counter;
    int32_t queued_pseudosymbols;          /* len(queued_pseudosymbols) */
    int64_t pseudosymbol_cursor_within_queue;
    int64_t slide;
    int64_t failed_bit_count;
    int64_t emitted_bit_count;
    int64_t processed_pseudosymbol_count;
    int32_t last_emitted_bits_len;         /* <= 50 */
    int8_t last_emitted_bits[52];          /* oldest first, GYP_BIT_* */
} gyp_bits_state;

int gyp_bits_create(int32_t n_channels, gyp_bits** out);
void gyp_bits_destroy(gyp_bits* bits);
int gyp_bits_reset(gyp_bits* bits, int32_t channel /* -1 = every channel */);
/* process_pseudosymbol (:267-288) for `n` consecutive pseudosymbols of one channel.  receiver_timestamp[i] is the
 * chunk.start_time the pipeline passes (pipeline.py:79); start/end are EmittedPseudosymbol.start_of_pseudosymbol /
 * end_of_pseudosymbol; pseudosymbol[i] is -1 or +1.  cursor_at_emit_out (may be NULL) receives the value the
 * reference stores into EmittedPseudosymbol.cursor_at_emit_time.  Emitted bits are appended to an internal FIFO;
 * up to `capacity` of them are moved to events_out (n_events_out = how many), the rest wait for gyp_bits_drain. */
int gyp_bits_push(gyp_bits* bits, int32_t channel, int32_t n, const double* receiver_timestamp,
                  const double* start_of_pseudosymbol, const double* end_of_pseudosymbol,
                  const int8_t* pseudosymbol, int32_t* cursor_at_emit_out, gyp_bit_event* events_out,
                  int32_t capacity, int32_t* n_events_out);
/* The same for a whole gyp_track_block output: recs_host is n_chan x n_ms (channel-major), channel c feeds
 * integrator c, visited millisecond by millisecond in channel order like receiver.py:244-247 visits its pipelines.
 * A channel stops being fed at its first record with status != 0 (the tracker raised LostSatelliteLockError before
 * the integrator saw that pseudosymbol).  start_time/end_time: n_ms chunk timestamps shared by all channels; each
 * pseudosymbol's edges are those plus (code_phase / 2046) ms as in tracker.py:319-326, and the chunk start is the
 * receiver timestamp (pipeline.py:79). */
int gyp_bits_push_block(gyp_bits* bits, const gyp_track_rec* recs_host, int32_t n_chan, int32_t n_ms,
                        const double* start_time, const double* end_time, gyp_bit_event* events_out,
                        int32_t capacity, int32_t* n_events_out);
int gyp_bits_drain(gyp_bits* bits, gyp_bit_event* events_out, int32_t capacity, int32_t* n_events_out);
int gyp_bits_get_state(const gyp_bits* bits, int32_t channel, gyp_bits_state* out);

/* ---------------------------------------------------------------- IQ ingest ---------------------------- */
/* SURVEY.md 8 f2.  Replaces the per-millisecond file open + np.fromfile of
 * antenna_sample_provider.py:79-136 AntennaSampleProviderBackedByFile (format of radio_input.py:22-44: interleaved
 * I,Q words, GNU Radio float32 by default): a reader thread preads blocks of `block_ms` milliseconds into a ring of
 * `depth` (pinned) host buffers; gyp_ingest_next_dev uploads them on a copy stream one block ahead of the consumer
 * and, for integer recordings, widens the words to float32 pairs on the device.  Sample values are exactly
 * `words[0::2] + 1j*words[1::2]` of the same dtype. */
typedef struct gyp_ingest gyp_ingest;

#define GYP_FMT_F32 0   /* numpy float32, GNU Radio recordings (radio_input.py:41) */
#define GYP_FMT_I8 1    /* numpy int8   (HackRF raw) */
#define GYP_FMT_I16 2   /* numpy int16 */
#define GYP_FMT_U8 3    /* numpy uint8  (RTL-SDR raw; no offset is removed, as np.fromfile would not: gyp_ingest_set_level / _calibrate do) */

/* ctx may be NULL: host-only reader (plain host buffers, gyp_ingest_next_host only).  n = samples per millisecond
 * (SampleProviderAttributes.samples_per_prn_transmission); block_ms >= 1; 3 <= depth <= 64. */
int gyp_ingest_open(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_hz, int32_t n, int32_t block_ms,
                    int32_t depth, gyp_ingest** out);
void gyp_ingest_close(gyp_ingest* ing);
/* Milliseconds the reference provider hands out before raising NoMoreSamplesError: it refuses a chunk whose end
 * offset is >= the file size (antenna_sample_provider.py:106), so a chunk ending exactly at EOF is not delivered. */
int64_t gyp_ingest_total_ms(const gyp_ingest* ing);
/* Integer recordings only: device samples become word * scale (one float32 multiply) for blocks uploaded from now
 * on.  The default 1 keeps the reference's raw integer values; the tracking loops' fixed thresholds and gains
 * (tracker.py:157-203,246-262) assume GNU-Radio-like amplitudes, so an 8-bit front end wants about 1/100 -- or a level measured
 * from the recording itself (gyp_ingest_calibrate, "level" below), which also removes an offset. */
int gyp_ingest_set_scale(gyp_ingest* ing, float scale);
/* Restart reading at millisecond `ms` (the provider's cursor / N). */
int gyp_ingest_seek(gyp_ingest* ing, int64_t ms);
/* Next block as raw file words on the host (n_ms x 2N words); valid until the next call on this handle.
 * *n_ms_out == 0 means end of data. */
int gyp_ingest_next_host(gyp_ingest* ing, const void** raw_out, int64_t* first_ms_out, int32_t* n_ms_out);
/* Host locality of the context's GPU: its NUMA node (-1: the host does not say) and that node's CPU list as sysfs prints it
 * ("0-31,128-159"; empty if unknown).  gyp_ingest_open allocates its pinned ring on that node and runs its reader thread there;
 * a multi-rank launcher (bench.py --gpus N) binds each rank's host thread the same way. */
int gyp_device_locality(gyp_ctx* ctx, int32_t* numa_node_out, char* cpulist_out, int32_t cap);
/* Next block as complex64 (interleaved float32 I,Q) in HBM, n_ms x N samples.  The context's stream is made to wait
 * for the upload, so kernels enqueued on it afterwards see the data; nothing blocks the host except waiting for the
 * reader thread.  The block stays valid while the next depth-2 calls are made.  *n_ms_out == 0: end of data. */
int gyp_ingest_next_dev(gyp_ingest* ing, const float** iq_dev_out, int64_t* first_ms_out, int32_t* n_ms_out);
/* AntennaSampleChunk.start_time / end_time of milliseconds first_ms .. first_ms+n_ms-1: round(cursor / fs, 6)
 * (antenna_sample_provider.py:88-89), bit-identical to Python's round(). */
int gyp_ingest_times(const gyp_ingest* ing, int64_t first_ms, int32_t n_ms, double* start_out, double* end_out);

/* ---------------------------------------------------------------- resampler ---------------------------- */
/* Recordings at any whole-kHz rate (RTL-SDR 2.048 Msps, USRP / bladeRF 4, 5, 10, 20, 25 Msps, ...) become a stream at the
 * context's format on the device; everything downstream then runs unchanged at that rate.  Opt-in: gyp_set_stream_format and
 * gyp_ingest_open still refuse such rates.
 *
 * Contract.  fs_in = N_in * 1000 Hz; fs_out = N_out * 1000 Hz is the context's stream format (GYP_E_NO_FORMAT if none is set)
 * or, for gyp_resample_design, the argument.  0.5 <= fs_out / fs_in <= 2 and fs_in != fs_out, else GYP_E_BAD_RATE.  taps T is
 * 16, 24, 32, 48 or 64 (0 = 32), else GYP_E_BAD_ARG.  Output millisecond m starts exactly at input sample m * N_in; its sample r
 * (0 <= r < N_out) is
 *     i0 = m*N_in + floor(r*N_in / N_out),   mu = ((r*N_in) mod N_out) / N_out
 *     y  = sum_{j = -T/2+1 .. T/2} h_mu[j] * x[i0 + j]
 *     h_mu[j] = c(j - mu) / sum_j' c(j' - mu),   c(t) = fc * sinc(fc*t) * I0(beta * sqrt(1 - (t/(T/2))^2)) / I0(beta),
 *     fc = 0.9 * min(fs_in, fs_out) / fs_in,  beta = 8,  sinc(x) = sin(pi x) / (pi x)
 * x is the recording, word * scale per component (integer formats widened as the ingest does), zero at indices below 0 and at or
 * beyond the last whole sample of the file or buffer.  Each phase has unit DC gain and is symmetric about the output instant:
 * output sample n lies at time n / fs_out (no delay), so a signal at code delay tau acquires at code phase round(tau * fs_out).
 * The design has L = N_out / gcd(N_in, N_out) phases (1023 for 2.048 -> 2.046, 4.0 -> 4.092, 5.0 -> 5.115, 10 -> 8.184).
 * Passband (float64 model, error of a complex tone <= 2e-4 of its amplitude): |f| <= B * min(fs_in, fs_out), measured at
 * ratios near 1, near 2 and at exactly 0.5, where the T input taps span only T/2 outputs and the band is narrowest:
 *         T    ratio near 1 or 2    ratio 0.5
 *        16          0.25              0.12
 *        24          0.30              0.20
 *        32          0.35              0.25
 *        48          0.35              0.30
 *        64          0.35              0.35
 * An output sample is a fixed function of its inputs (one float32 fma chain in tap order, whatever the call's window, block or
 * launch shape): blocks, windows and seeks give bit-identical samples. */

/* Host only (no GPU): writes the L x T float32 design, row p = mu * L (phase-major), computed in float64 and rounded.  table_out
 * NULL: only *n_phases_out = L is written. */
int gyp_resample_design(int64_t fs_in_hz, int64_t fs_out_hz, int32_t taps, float* table_out, int32_t* n_phases_out);
/* raw_dev holds n_streams streams of interleaved I,Q words of format fmt (GYP_FMT_*), stream s at raw_dev + s * in_stride_samples
 * samples; its sample 0 is input sample raw_first_sample (may be negative), and only raw_n_samples of them (<= in_stride_samples)
 * exist: the rest read as zero.  Writes output milliseconds first_ms .. first_ms+n_ms-1 of every stream, complex64, stream s at
 * out_dev + s * out_stride_samples samples (>= n_ms * N_out).  Enqueued on the context's stream; the design is built on first
 * use of each (fs_in, fs_out, taps) and cached on the context. */
int gyp_resample_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, int32_t n_streams, int64_t in_stride_samples,
                        int64_t raw_first_sample, int64_t raw_n_samples, float scale, int64_t fs_in_hz, int32_t taps, int64_t first_ms,
                        int32_t n_ms, int64_t out_stride_samples, float* out_dev);
/* An ingest handle over a recording at fs_in_hz whose device blocks are at the context's rate (ctx required).  The reader preads
 * each block's input span plus its (T-1)-sample halo (zero beyond the file's edges); the upload stream runs the resampler where
 * it would run the widen kernel.  gyp_ingest_total_ms applies gyp_ingest_open's rule ((size - 1) / input millisecond bytes) to the
 * input file; gyp_ingest_times gives round(k * N_out / fs_out, 6); set_scale, seek, next_dev and close keep their meaning;
 * gyp_ingest_next_host returns GYP_E_BAD_ARG. */
int gyp_ingest_open_resampled(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_in_hz, int32_t taps, int32_t block_ms,
                              int32_t depth, gyp_ingest** out);

/* ---------------------------------------------------------------- down-converter ----------------------- */
/* Real-sampled recordings at an intermediate frequency (MAX2769-style front ends: 16.368 Msps, IF 4.092 MHz; the classic int8
 * data set: 38.192 Msps, IF 9.548 MHz) become complex baseband at the context's format on the device: a mixer in front of the
 * resampler's filter.
 *
 * Contract.  The input is one real word per sample, of format fmt (GYP_FMT_*): x[i] = word[i] * scale, integer formats widened
 * as the ingest does; x is zero at indices below 0 and at or beyond the last sample of the buffer or file.  fs_in = N_in * 1000
 * Hz; fs_out = N_out * 1000 Hz is the context's stream format (GYP_E_NO_FORMAT if none is set) or, for gyp_ddc_design, the
 * argument.  if_hz is a signed whole number of Hz.
 *     z[i] = x[i] * exp(-j theta_i),   theta_i = 2 pi ((if_hz * i) mod fs_in) / fs_in
 * with i the absolute input index (from sample 0 of the file or buffer) and the reduction exact integer arithmetic, so windows,
 * blocks and seeks see the same mixer value at the same i, whatever i (2^43 included).  The device evaluates each mixer value in
 * float32 within 2^-22 of the exact one.  Output sample r of millisecond m is
 *     y = sum_{j = -T/2+1 .. T/2} h_mu[j] * z[i0 + j]
 * with i0, mu, h_mu and the tap range exactly the resampler's (fc = 0.9 * fs_out / fs_in, since fs_out < fs_in here).  There is
 * no factor 2: a real tone A cos(2 pi (if_hz + d) t + phi) comes out as (A/2) exp(j (2 pi d t + phi)).  A negative if_hz selects
 * the mirrored band: that is how a spectrally inverted (high-side LO) recording is read, a satellite at Doppler +d coming out at +d.
 * Rates, checked in integers, else GYP_E_BAD_RATE: both whole kHz, fs_in < 2^31 Hz, 8 fs_out >= fs_in, 20 |if_hz| >= 9 fs_out
 * (the mirror band at -2 if_hz clears the +-0.45 fs_out passband) and 20 |if_hz| + 9 fs_out <= 10 fs_in (the band lies below the
 * real Nyquist frequency); together fs_out / fs_in <= 5/9, and if_hz = 0 is refused.  Admitted, e.g.: 16.368 Msps at IF
 * +-4.092 MHz to 4.092 and 8.184 Msps; 38.192 Msps at IF 9.548 MHz to 8.184 and 16.368 Msps; 5 Msps at IF 1.25 MHz to 2.046 Msps.
 * Taps T is 32, 48, 64, 96 or 128, else GYP_E_BAD_ARG; T = 0 picks the smallest with T * fs_out >= 16 * fs_in (the filter spans at
 * least 16 output samples; the ratio bound 1/8 makes 128 always enough): 64 at 16.368 -> 4.092, 96 at 38.192 -> 8.184.
 * Passband by the number of output samples the filter spans, T * fs_out / fs_in (float64 model: a real tone at if_hz + d with
 * |d| <= B * fs_out comes out within 2e-4 of A/2, its mirror included; measured at ratios 1/8, 1/4 and 1/2):
 *        T * ratio      6     8    12    16    24    32
 *        B           0.02  0.12  0.23  0.29  0.34  0.37
 * (below 0.01 at T * ratio = 4, which T = 32 gives at the ratio bound 1/8; T = 0 always spans 16 or more.)
 * Each output is one float32 fma chain in tap order over mixed inputs that depend on i alone: blocks, windows,
 * seeks and launch shapes give bit-identical samples. */

/* Host only (no GPU): validates the rules above and writes the L x T float32 design in the resampler's layout (row p = mu * L),
 * computed in float64 and rounded; *taps_out receives the T that 0 resolves to.  Any of the outputs may be NULL. */
int gyp_ddc_design(int64_t fs_in_hz, int64_t fs_out_hz, int64_t if_hz, int32_t taps, float* table_out, int32_t* n_phases_out,
                   int32_t* taps_out);
/* As gyp_resample_iq_dev, with one real word per sample: strides count real samples, and raw_first_sample is the absolute index
 * the mixer phase uses.  The design is cached on the context next to the resampler's. */
int gyp_ddc_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, int32_t n_streams, int64_t in_stride_samples, int64_t raw_first_sample,
                   int64_t raw_n_samples, float scale, int64_t fs_in_hz, int64_t if_hz, int32_t taps, int64_t first_ms, int32_t n_ms,
                   int64_t out_stride_samples, float* out_dev);
/* An ingest handle over a real recording at fs_in_hz whose device blocks are complex baseband at the context's rate (ctx required).
 * The input millisecond is N_in * word bytes; the halo is T-1 samples and the mixer index of each staged sample is its absolute
 * index in the file.  total_ms, times, set_scale, seek, next_dev and close behave as for a resampled handle; gyp_ingest_next_host
 * returns GYP_E_BAD_ARG. */
int gyp_ingest_open_ddc(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_in_hz, int64_t if_hz, int32_t taps, int32_t block_ms,
                        int32_t depth, gyp_ingest** out);

/* ---------------------------------------------------------------- packed recordings -------------------- */
/* Dedicated GNSS front ends (MAX2769-class boards) and many published data sets store 1-, 2- or 4-bit words packed into bytes:
 * files 2-8 times smaller than int8.  They cross PCIe packed and are unpacked on the device, by the kernels that widen words
 * elsewhere: native-rate I,Q (gyp_unpack_iq_dev), the resampler and the down-converter (gyp_resample_packed_dev).
 *
 * Contract.  Word w of the file occupies bits [w * bits, (w + 1) * bits) of the byte stream: byte (w * bits) / 8, and within
 * that byte the earliest word sits in the most significant bits (GYP_PACK_MSB_FIRST) or in the least (GYP_PACK_LSB_FIRST).
 * 2-bit MSB-first, byte 0b00011011 holds codes 0, 1, 2, 3 in that order; LSB-first it holds 3, 2, 1, 0.  The value of word w
 * is levels[code] * scale, one float32 multiply, exactly as (float)word * scale is for the byte-wide formats.  real = 0: words
 * alternate I, Q and a sample is 2 words; real = 1: one real word per sample at an intermediate frequency.  A sample spans
 * B = bits * (2 - real) bits, which divide 8, so no sample straddles a byte.  file_samples = floor(8 * size / B): the
 * trailing bits of a partial sample are ignored.  The file's milliseconds follow gyp_ingest_open's rule counted in samples,
 * total_ms = (file_samples - 1) / N_in, which equals (size - 1) / ms_bytes of the int8 file holding the same words.
 * Millisecond and block edges need not fall on byte boundaries: a buffer starts bit0 bits into its first byte (bit0 a
 * multiple of B below 8), and samples outside the buffer's raw_n_samples, or outside the file, are zero by index -- never
 * the level of a zero-filled byte (code 0 is +1 under sign-magnitude).  With those values, packed results are bit-identical to
 * the int8 path on a file whose words are the levels. */
#define GYP_PACK_MSB_FIRST 0   /* the earliest word of a byte sits in its most significant bits */
#define GYP_PACK_LSB_FIRST 1
typedef struct gyp_packing {
    int32_t bits;       /* 1, 2 or 4 bits per word */
    int32_t real;       /* 0: words alternate I, Q (a sample = 2 words); 1: one real word per sample (IF recordings) */
    int32_t order;      /* GYP_PACK_MSB_FIRST / GYP_PACK_LSB_FIRST */
    int32_t reserved;   /* must be 0 */
    float levels[16];   /* value of code c, 0 <= c < 2^bits, before scale; finite; entries >= 2^bits ignored */
} gyp_packing;
/* Host only (no GPU): where samples first_sample .. first_sample + n_samples - 1 (first_sample may be negative) lie in a file
 * of file_bytes bytes.  Only the part inside [0, file_samples) is read: *in_first_out / *in_n_out are that part (in_n 0 if none),
 * and *first_byte_out, *bit0_out, *n_bytes_out the bytes that cover it and the bit offset of its first sample in the first
 * byte.  *file_samples_out and *total_ms_out (samples_per_ms = N_in) follow the contract.  Any output may be NULL.  The ingest
 * reads exactly these bytes.  GYP_E_BAD_ARG for an invalid packing, n_samples < 0, file_bytes < 0 or samples_per_ms < 1. */
int gyp_packed_span(const gyp_packing* packing, int32_t samples_per_ms, int64_t file_bytes, int64_t first_sample, int64_t n_samples,
                    int64_t* in_first_out, int64_t* in_n_out, int64_t* first_byte_out, int32_t* bit0_out, int64_t* n_bytes_out,
                    int64_t* file_samples_out, int64_t* total_ms_out);
/* Packed I,Q words (real = 0 only) -> complex64 at their own rate, on the context's stream.  Stream s starts at byte
 * raw_dev + s * in_stride_bytes, its sample 0 bit0 bits into that byte; n_samples samples are written per stream, stream s at
 * out_dev + s * out_stride_samples.  in_stride_bytes must hold bit0 + n_samples * B bits.  Equal, bit for bit, to
 * gyp_widen_iq_dev on the int8 words holding the levels. */
int gyp_unpack_iq_dev(gyp_ctx* ctx, const gyp_packing* packing, const void* raw_dev, int32_t n_streams, int64_t in_stride_bytes,
                      int32_t bit0, int64_t n_samples, float scale, int64_t out_stride_samples, float* out_dev);
/* gyp_resample_iq_dev (real = 0, if_hz must be 0) or gyp_ddc_iq_dev (real = 1, if_hz required) on packed words: the packing in
 * place of fmt, strides in bytes, and the bit offset of the buffer's sample 0 (raw_first_sample) in its first byte.  Same rate,
 * tap and error rules, same cached designs, bit-identical to the int8 path on the words holding the levels. */
int gyp_resample_packed_dev(gyp_ctx* ctx, const gyp_packing* packing, const void* raw_dev, int32_t n_streams, int64_t in_stride_bytes,
                            int32_t bit0, int64_t raw_first_sample, int64_t raw_n_samples, float scale, int64_t fs_in_hz, int64_t if_hz,
                            int32_t taps, int64_t first_ms, int32_t n_ms, int64_t out_stride_samples, float* out_dev);
/* An ingest handle over a packed recording (ctx required).  I,Q at the context's rate: unpacked only (taps ignored); I,Q at another
 * whole-kHz rate: resampled; real: down-converted, if_hz required (and 0 for I,Q).  The reader preads the bytes that cover each
 * block's samples (gyp_packed_span) and the upload stream unpacks them; there is no repacking on the host.  total_ms follows
 * the contract; times, set_scale, seek, next_dev and close keep their meaning; gyp_ingest_next_host returns GYP_E_BAD_ARG.
 * GYP_E_BAD_ARG for bits not 1, 2 or 4, reserved != 0, an unknown order, a non-finite level, real without if_hz or I,Q with one;
 * the rate rules return GYP_E_BAD_RATE as for the other handles. */
int gyp_ingest_open_packed(gyp_ctx* ctx, const char* path, const gyp_packing* packing, int64_t fs_in_hz, int64_t if_hz, int32_t taps,
                           int32_t block_ms, int32_t depth, gyp_ingest** out);

/* ---------------------------------------------------------------- level: DC offset and amplitude ------- */
/* Offset-binary recordings (RTL-SDR uint8, zero at 128) carry a DC term far above the noise, and the tracking loops' fixed
 * thresholds assume GNU-Radio-like amplitudes.  Three steps condition a recording on the device: measure per-millisecond
 * statistics (gyp_iq_stats_dev), derive a level from them on the host (gyp_iq_level_from_stats), apply it (gyp_condition_iq_dev,
 * or gyp_ingest_set_level / gyp_ingest_calibrate on an ingest handle).  Everything is opt-in: with none of these called every
 * other entry point gives the bits it gave before.
 *
 * Statistics.  One record per (stream, millisecond), a pure function of that millisecond's samples: reduced in a fixed order with
 * a fixed lane-to-sample mapping and a fixed tree (in-wave, then across waves through LDS), without floating-point atomics, so
 * the same bits come out on every run and for every call shape -- other n_streams / n_ms, a sub-window of the same buffer,
 * another grid size, whatever the rows' alignment.  Products and sums are single float64 roundings; for integer-valued samples
 * with |v| < 2^15 every partial sum is an exact integer below 2^53 and the sums equal numpy's int64 sums.  Non-finite samples:
 * the sums follow IEEE; max_abs and n_clip are unspecified. */
typedef struct gyp_iq_stats {   /* one per (stream, millisecond): 32 bytes */
    double sum_re, sum_im;      /* sum of Re x, Im x over the millisecond's samples, accumulated in float64 */
    double sum_sq;              /* sum of (Re x)^2 + (Im x)^2, products and sums in float64 */
    float  max_abs;             /* max over samples of max(|Re x|, |Im x|) */
    int32_t n_clip;             /* COMPONENTS with |v| >= clip_level; 0 when clip_level <= 0 */
} gyp_iq_stats;
/* iq_dev: n_streams x n_ms x samples_per_ms complex64 samples, stream s at sample s * stream_stride_samples; any 8-byte aligned
 * address and any stride (rows that start on 16 bytes are read 16 bytes at a time, the others 8).  samples_per_ms is an argument
 * (>= 1), no stream format is needed: the function also works on data at a recording's own rate.  out_dev: n_streams x n_ms
 * records, stream-major.  Enqueued on the context's stream.  GYP_E_BAD_ARG for NULL pointers, counts < 1, or a stride below
 * n_ms * samples_per_ms when n_streams > 1. */
int gyp_iq_stats_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     int32_t samples_per_ms, float clip_level, gyp_iq_stats* out_dev);

/* y_re = (x_re - dc_re) * gain, y_im = (x_im - dc_im) * gain: one float32 subtraction, then one float32 multiplication, each
 * rounded to nearest -- what numpy computes for (x - dc) * g in float32.  The level {0, 0, 1} returns the input bits. */
typedef struct gyp_iq_level {
    float dc_re, dc_im;   /* finite */
    float gain;           /* positive and finite */
    int32_t reserved;     /* must be 0 */
} gyp_iq_level;
/* n_samples samples of each of n_streams streams (stream s at sample s * stream_stride_samples of both buffers), stream s with
 * levels_host[s].  out_dev may equal in_dev; other overlaps are not allowed.  Alignment as for gyp_iq_stats_dev.  Enqueued on the
 * context's stream; levels_host may be reused as soon as the call returns.  GYP_E_BAD_ARG for NULL pointers, n_streams < 1,
 * n_samples < 0, a stride below n_samples when n_streams > 1, or a level that breaks the rules above. */
int gyp_condition_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples,
                         int64_t n_samples, const gyp_iq_level* levels_host);

/* Host only (no GPU; errors through gyp_last_error(NULL)): the level that removes the mean (remove_dc != 0) and brings the RMS of
 * |x| per complex sample to target_rms, from n_ms records of one stream.  Float64, in exactly this order, one rounding per
 * operation (no contraction):
 *     S_re, S_im, S_sq = the plain left-to-right sums of sum_re, sum_im, sum_sq over the records;  C = the int64 sum of n_clip
 *     M = (double)n_ms * samples_per_ms;   m_re = S_re / M;   m_im = S_im / M;   P = S_sq / M
 *     (d_re, d_im) = remove_dc ? (m_re, m_im) : (0, 0)
 *     a = d_re * d_re;   b = d_im * d_im;   q = a + b;   V = P - q;   rms = sqrt(V);   g = target_rms / rms
 * level_out = {(float)d_re, (float)d_im, (float)g, 0};  measured_out4 (may be NULL) = {m_re, m_im, rms, C / (2 M)}: the mean, the
 * RMS about the removed offset and the share of clipped components.  GYP_E_BAD_ARG for NULL stats or level_out, n_ms < 1,
 * samples_per_ms < 1, target_rms not positive and finite, V not positive and finite (a constant recording has no power to
 * scale), or a level that float32 cannot hold. */
int gyp_iq_level_from_stats(const gyp_iq_stats* stats, int32_t n_ms, int32_t samples_per_ms, int32_t remove_dc, double target_rms,
                            gyp_iq_level* level_out, double* measured_out4);

/* A level on an ingest handle (ctx required: a host-only handle returns GYP_E_BAD_ARG from all three, and gyp_ingest_next_host
 * returns GYP_E_BAD_ARG while a level is on -- host blocks are raw file words, which a level does not define).  Where a level is
 * on, every device block is conditioned in place on the upload stream, behind whatever produced it (the widen, unpack, resample
 * or down-convert kernel, or the plain copy of a float32 recording): its samples are exactly gyp_condition_iq_dev of the samples
 * the handle delivers without a level -- sample = word * scale as before, then the level.  The level is a constant of the handle,
 * not a per-block estimate, so blocks, windows and seeks keep giving bit-identical samples.
 * gyp_ingest_set_level (NULL: off) takes effect with the next block handed out: what was uploaded ahead is dropped and read
 * again, as a seek to the consumer's position does. */
int gyp_ingest_set_level(gyp_ingest* ing, const gyp_iq_level* level);
int gyp_ingest_get_level(const gyp_ingest* ing, gyp_iq_level* out, int32_t* enabled_out);
/* Measures output milliseconds [first_ms, first_ms + n_ms) of the handle, which must lie in [0, total_ms) with 1 <= n_ms <= 10000,
 * and installs the level gyp_iq_level_from_stats derives.  What is measured is the handle's UNCONDITIONED output: the samples it
 * delivers with its current scale (sample = word * scale) and without a level, whether or not one is installed.  The blocks are
 * read through the handle's own path, gyp_iq_stats_dev (clip_level as given) runs on them and the records are combined in
 * millisecond order, so the level does not depend on block_ms.  The cursor is put back where it was; the call synchronises, and
 * blocks handed out earlier are no longer valid afterwards.  level_out / measured_out4 (either may be NULL) receive what
 * gyp_iq_level_from_stats wrote.  On an error the handle keeps the level it had.
 * With a blanker installed ("blanker" below), and only then, what is measured is the BLANKED output (and, as before, the notched
 * one where notches are installed): the chain is producer -> blanker -> notches -> level, and an RMS taken under pulses is useless. */
int gyp_ingest_calibrate(gyp_ingest* ing, int64_t first_ms, int32_t n_ms, int32_t remove_dc, double target_rms, float clip_level,
                         gyp_iq_level* level_out, double* measured_out4);

/* ---------------------------------------------------------------- notch: narrowband (CW) interference -- */
/* A CW spur inside the band (a harmonic of an RTL-SDR's 28.8 MHz reference, a USB or clock spur, a jammer) far above the noise
 * jams every Doppler bin.  The level above removes one frequency, 0 Hz; these calls find and remove tones at any whole number of
 * Hz with |f| < fs / 2.  Everything is opt-in: with none of them called every other entry point gives the bits it gave before.
 *
 * Phase.  theta(i) = 2 pi ((f i) mod fs) / fs, i the ABSOLUTE index of the sample in its stream (first_sample_index + its offset
 * in the buffer), reduced in integers; the device uses the float32 pair (cos theta, sin theta) of the down-converter's mixer,
 * within 2^-22 of exact at any index and a pure function of (f, i).  fs_hz must lie in [1000, 2^31).
 *
 * Measurement (gyp_iq_tones_dev).  For each (stream, block b, frequency f) one record
 *     A = (sum_n w[n] x[i0 + n] e^(-j theta(i0 + n))) / sum_n w[n],       i0 = first_sample_index + b * block_samples
 * over the block's block_samples samples, w = 1 (GYP_WINDOW_RECT) or w[n] = sin^2(pi (n + 1) / (B + 1)) (GYP_WINDOW_HANN: nonzero
 * on every sample; its sum is (B + 1) / 2, which is what the device divides by).  Products and sums are float64 over the float32
 * mixer value: per sample (x_re c - x_im s', x_re s' + x_im c) with s' = -sin theta (the four products are exact, the difference
 * and the sum one rounding each), times w[n] (Hann only), added to the owning thread's accumulator.  Thread t of 256 owns samples
 * n = t, t + 256, ...; the partial sums are reduced by a fixed tree (in-wave, then across the wavefronts through LDS), without
 * floating-point atomics and without contraction, as the statistics above: the same record bits for every grid size, every
 * sub-window of the same buffer (same absolute indices) and every row alignment. */
typedef struct gyp_tone_rec {   /* 16 bytes */
    double re, im;
} gyp_tone_rec;
#define GYP_WINDOW_RECT 0
#define GYP_WINDOW_HANN 1
#define GYP_NOTCH_MAX_TONES 8
/* iq_dev: complex64, stream s at sample s * stream_stride_samples, any 8-byte aligned address; no stream format is needed.
 * freqs_hz_host: n_freq whole Hz, |f| < fs / 2 (copied before the call returns).  out_dev: n_streams x n_blocks x n_freq records,
 * stream-major, then block, then frequency.  Enqueued on the context's stream (the call waits for the upload of the frequency
 * list).  GYP_E_BAD_ARG for NULL pointers, counts < 1, first_sample_index < 0, a stride below n_blocks * block_samples when
 * n_streams > 1, an fs_hz or a frequency out of range, or a window that is neither of the two. */
int gyp_iq_tones_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_sample_index,
                     int32_t n_blocks, int32_t block_samples, int64_t fs_hz, const int64_t* freqs_hz_host, int32_t n_freq, int32_t window,
                     gyp_tone_rec* out_dev);

/* Removal.  Per (stream, millisecond of samples_per_ms samples) and for the stream's tones t = 0 .. count-1 IN LIST ORDER -- a
 * sequential projection:
 *     A_t = the rectangular measurement above over the millisecond, taken on the residual y_(t-1) that tones 0 .. t-1 left
 *           (y_(-1) = x; 1024 threads: thread t owns samples t, t + 1024, ...), then a = ((float)Re A_t, (float)Im A_t)
 *     y_t = y_(t-1) - a e^(+j theta_t) in float32:  p_re = a_re c - a_im s,  p_im = a_re s + a_im c  (four products, then the
 *           difference and the sum), y_re = y_re - p_re, y_im = y_im - p_im: one float32 rounding per operation, no contraction.
 * The amplitude is a per-millisecond estimate, the frequencies are constants of the call: the same samples come out for every
 * n_streams / n_ms split, window and grid size.  A tone 50 Hz off its listed frequency is still suppressed by about 20 dB
 * (|1 - sinc|-like residual of a one-millisecond projection); re-run gyp_ingest_find_tones for recordings that drift further.
 * The projection also takes the part of the wanted signal that lies on the tone: 1 / samples_per_ms of the power per tone.
 * An empty list returns the input bits.  out_dev may equal in_dev; other overlaps are not allowed. */
typedef struct gyp_notch_tones {   /* one per stream: 72 bytes */
    int32_t count;                 /* 0 .. GYP_NOTCH_MAX_TONES */
    int32_t reserved;              /* must be 0 */
    int64_t freq_hz[GYP_NOTCH_MAX_TONES];   /* |f| < fs / 2, pairwise at least 4000 Hz apart (over 1 ms closer tones are far from orthogonal) */
} gyp_notch_tones;
/* Enqueued on the context's stream; tones_host (n_streams records) may be reused as soon as the call returns.  GYP_E_BAD_ARG for
 * NULL pointers, n_streams < 1, n_ms < 0, samples_per_ms < 1, first_sample_index < 0, a stride below n_ms * samples_per_ms when
 * n_streams > 1, fs_hz out of range, or a tone list that breaks the rules above (count > 8, |f| >= fs / 2, two tones closer than
 * 4000 Hz, reserved != 0). */
int gyp_notch_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples,
                     int64_t first_sample_index, int32_t n_ms, int32_t samples_per_ms, int64_t fs_hz, const gyp_notch_tones* tones_host);

/* Host only (no GPU; errors through gyp_last_error(NULL)).  The tones of a power spectrum power[0 .. n_freq) whose bins are
 * freq_step_hz apart: bin k is a candidate if power[k] >= threshold_over_median * median(power) (the median of numpy: the mean of
 * the two middle values for an even count), power[k] > 0, power[k] > power[k-1] (or k = 0) and power[k] >= power[k+1] (or
 * k = n_freq - 1) -- of equal neighbours the lowest bin is the maximum.  Candidates are taken strongest first, of equal powers
 * the lowest bin first; one that lies closer than min_separation_bins to a bin already taken is dropped; at most max_tones are
 * written to out_bins.  Returns their number (>= 0), or GYP_E_BAD_ARG for NULL pointers, n_freq < 1, a power that is negative or
 * not finite, a threshold or freq_step_hz that is not positive and finite, min_separation_bins < 1 or max_tones < 0. */
int gyp_tones_find(const double* power, int32_t n_freq, double freq_step_hz, double threshold_over_median, int32_t min_separation_bins,
                   int32_t max_tones, int32_t* out_bins);
/* Host only.  The frequency offset of a tone from the frequency its records were measured at (n_blocks >= 2 consecutive blocks
 * of block_seconds each), as the phase slope: float64, in exactly this order, one rounding per operation:
 *     S = sum over b = 0 .. n_blocks-2, left to right, of A[b+1] conj(A[b]):
 *         c_re = A[b+1].re A[b].re + A[b+1].im A[b].im,   c_im = A[b+1].im A[b].re - A[b+1].re A[b].im
 *     *delta_hz_out = atan2(S_im, S_re) / (6.283185307179586 * block_seconds)
 * Valid for |delta| < 1 / (2 block_seconds).  GYP_E_BAD_ARG for NULL pointers, n_blocks < 2 or block_seconds not positive and finite. */
int gyp_tone_refine(const gyp_tone_rec* records, int32_t n_blocks, double block_seconds, double* delta_hz_out);

/* Notches on an ingest handle (ctx required: a host-only handle returns GYP_E_BAD_ARG from all of these, and gyp_ingest_next_host
 * returns GYP_E_BAD_ARG while notches are on).  CHAIN ORDER of a handle: producer (widen / unpack / resample / down-convert /
 * copy) -> notches -> level.  Every device block is notched in place on the upload stream exactly as gyp_notch_iq_dev would, at
 * the handle's output rate and with first_sample_index = the block's first millisecond * N, and conditioned with the level
 * afterwards.  gyp_ingest_calibrate therefore measures the NOTCHED output when notches are installed, and only then: a level
 * measured under a 40 dB jammer is useless, so find and install the tones first.
 * gyp_ingest_set_notches (n = 0 or freqs_hz NULL: off) follows gyp_ingest_set_level: it takes effect with the next block handed
 * out, and what was uploaded ahead is dropped and read again.  gyp_ingest_get_notches writes up to 8 frequencies and their count. */
int gyp_ingest_set_notches(gyp_ingest* ing, const int64_t* freqs_hz, int32_t n);
int gyp_ingest_get_notches(const gyp_ingest* ing, int64_t* freqs_out8, int32_t* n_out);
/* Finds the tones in output milliseconds [first_ms, first_ms + n_ms) of the handle (inside [0, total_ms), 1 <= n_ms <= 1000).
 * What is searched is the handle's output WITHOUT notches and without a level, read through the handle's own path into one
 * buffer, so the result does not depend on block_ms; the cursor is put back, the call synchronises, and blocks handed out
 * earlier are no longer valid afterwards.  Steps:
 *   1. scan: gyp_iq_tones_dev with Hann blocks of 1024 samples at the 1843 frequencies round(k fs / 2048) Hz, |k| <= 921
 *      (+-0.45 fs); the spectrum is the mean over the blocks, in block order, of re^2 + im^2 per frequency (float64);
 *   2. gyp_tones_find on it with `threshold` over the median and a separation of ceil(4000 / (fs / 2048)) + 2 grid points (the refinement
 *      moves a tone by less than one, so refined tones stay 4000 Hz apart) and up to 256 candidates.  A
 *      candidate is then dropped if it lies within 4 grid points of 0 Hz (the offset is the level's to remove:
 *      gyp_ingest_calibrate) or if its power is at most 4 times what the Hann window leaks there from 0 Hz or from a stronger
 *      tone already kept (bound: (pi x (x^2 - 1))^-2 of the peak at x = distance / 2 grid points >= 2); the strongest max_tones
 *      (<= 8) remain, strongest first;
 *   3. each is refined twice with gyp_tone_refine and rounded to whole Hz after each step: on Hann blocks of 64 samples (range
 *      +-fs / 128; Hann, so that the offset and stronger tones do not leak into a weak tone's records), then on rectangular
 *      blocks of one millisecond (needs n_ms >= 2; skipped otherwise).
 * freqs_out / power_db_out (room for max_tones; either may be NULL) receive the frequencies and 10 log10(power / median) of the
 * scan; *n_out their number.  With install != 0 the tones are installed as gyp_ingest_set_notches does (none found: notches off).
 * On an error the handle keeps the notches it had.
 * With a blanker installed ("blanker" below), and only then, what is searched is the BLANKED output, still without notches and
 * without a level: the blanker stands in front of the notches, and a per-millisecond projection taken under pulses is useless. */
int gyp_ingest_find_tones(gyp_ingest* ing, int64_t first_ms, int32_t n_ms, double threshold, int32_t max_tones, int32_t install,
                          int64_t* freqs_out, double* power_db_out, int32_t* n_out);

/* ---------------------------------------------------------------- blanker: pulsed interference ---------- */
/* Wideband pulses (radar, DME-like bursts, ignition noise, a neighbouring transmitter keying up, ADC saturation bursts) are
 * broadband, so a notch does nothing to them, and brief, so an RMS-based level is wrong in both directions: the pulses inflate
 * the RMS and the gain that follows crushes the satellites.  A pulse blanker replaces the samples of a pulse by the recording's
 * centre.  Three steps: a histogram of the power about the centre on the device (gyp_iq_power_hist_dev), a threshold from its
 * median on the host (gyp_blank_from_hist), the blanking (gyp_blank_iq_dev, or gyp_ingest_set_blanker / gyp_ingest_find_pulses
 * on an ingest handle).  Everything is opt-in: with none of these called every other entry point gives the bits it gave before.
 *
 * Decision.  Per (stream, millisecond of samples_per_ms samples), a pure function of that millisecond's samples.  In float32, one
 * rounding per operation, no contraction:
 *     dx = re - center_re;  dy = im - center_im;  a = dx dx;  b = dy dy;  p = a + b;  t2 = threshold threshold
 * Sample i is a HIT iff p >= t2 (equality is a hit; a NaN p is not).  Sample i is BLANKED iff some hit j of the SAME millisecond
 * has |i - j| <= guard.  A blanked sample becomes exactly (center_re, center_im); every other sample keeps its bits.
 * Guards do not cross millisecond edges, so blocks, windows, seeks and call shapes give identical samples, as the notch's
 * per-millisecond estimate does.  The cost: a hit within `guard` samples of an edge does not reach into the neighbouring
 * millisecond, so up to `guard` samples of a pulse's skirt on the other side of the edge stay. */
typedef struct gyp_blanker {      /* one per stream: 16 bytes */
    float center_re, center_im;   /* finite: the recording's offset (0 for float32 / int8; ~127.4 for offset-binary uint8) */
    float threshold;              /* positive, finite: amplitude about the centre */
    int32_t guard;                /* 0..64 samples blanked on either side of every hit */
} gyp_blanker;
#define GYP_POWER_HIST_BINS 2048
/* n_ms milliseconds of each of n_streams streams (stream s at sample s * stream_stride_samples of both buffers), stream s with
 * blankers_host[s].  out_dev may equal in_dev (then only blanked samples are written: one read of the block and a few percent of
 * a write); other overlaps are not allowed.  counts_out_dev (may be NULL) receives n_streams x n_ms int32 counts of blanked
 * samples per millisecond, stream-major.  Alignment as for gyp_iq_stats_dev: any 8-byte aligned address and any stride; rows that
 * start on 16 bytes (in both buffers) are read 16 bytes at a time.  samples_per_ms is an argument, no stream format is needed.
 * Enqueued on the context's stream; blankers_host may be reused as soon as the call returns.  GYP_E_BAD_ARG, before anything is
 * launched, for NULL pointers, n_streams < 1, samples_per_ms < 1 or > 65536, n_ms < 0, a stride below n_ms * samples_per_ms when
 * n_streams > 1, a centre that is not finite, a threshold that is not positive and finite, or a guard outside 0..64. */
int gyp_blank_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     int32_t samples_per_ms, const gyp_blanker* blankers_host, int32_t* counts_out_dev);

/* The histogram of p (as above, about centers_host[2 s], centers_host[2 s + 1]; NULL: 0) over n_samples samples of each stream:
 * n_streams x GYP_POWER_HIST_BINS uint32 counts into hist_out_dev, which the call zeroes first.  The bin of a sample is the bits
 * of p without the sign, shifted right by 20 -- 8 exponent bits and 3 mantissa bits: eighth-octave bins; p is never negative, and
 * a NaN's sign is not defined.  The lower edge of bin k is the float whose bits are k << 20.  Non-finite p lands in bins >= 2040
 * (+inf in 2040, NaN above).  Counts are integers, added with integer atomics: the same bits for every grid size, split and
 * alignment, and histograms of parts of a stream add up to the whole's.  Enqueued on the context's stream.  GYP_E_BAD_ARG for NULL
 * pointers (centers_host may be NULL), n_streams < 1, n_samples < 1, a stride below n_samples when n_streams > 1, or a centre that
 * is not finite. */
int gyp_iq_power_hist_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t n_samples,
                          const float* centers_host, uint32_t* hist_out_dev);

/* Host only (no GPU; errors through gyp_last_error(NULL)): the blanker whose threshold is sqrt(threshold_over_median x the median
 * of p) from one stream's histogram.  Float64, in exactly this order, one rounding per operation:
 *     M = the sum of bins 0 .. 2039 (the finite powers);   r = M / 2
 *     k = the first bin whose cumulative count cum_k = h_0 + .. + h_k is >= r;   lo_k = the lower edge of bin k
 *     median = lo_k + ((r - cum_(k-1)) / h_k) * (lo_(k+1) - lo_k)        (linear inside the bin)
 *     t = sqrt(threshold_over_median * median)
 * blanker_out = {center_re, center_im, (float)t, guard};  measured_out2 (may be NULL) = {median, t}.
 * What the median means: for complex Gaussian noise p is exponential and P(p > 16 median) = 2^-16, so a factor of 16 blanks one
 * clean sample in 65536.  Strong pulses of duty d push the estimate to the 0.5 / (1 - d) quantile of the noise: +17 % at d = 0.1,
 * where a factor of 16 acts like about 19; usable to a duty of roughly 40 %.  An eighth-octave bin is 9 % wide; the interpolation
 * brings the estimate to within about 1 %.
 * GYP_E_BAD_ARG for NULL hist or blanker_out, M = 0, a median that is not positive, a factor that is not positive and finite, a
 * centre that is not finite, a guard outside 0..64, or a threshold that float32 cannot hold. */
int gyp_blank_from_hist(const uint32_t* hist, float center_re, float center_im, double threshold_over_median, int32_t guard,
                        gyp_blanker* blanker_out, double* measured_out2);

/* A blanker on an ingest handle (ctx required: a host-only handle returns GYP_E_BAD_ARG from all four, and gyp_ingest_next_host
 * returns GYP_E_BAD_ARG while a blanker is on).  CHAIN ORDER of a handle: producer (widen / unpack / resample / down-convert /
 * copy) -> blanker -> [excisor, below ->] notches -> level.  Every device block is blanked in place on the upload stream exactly as gyp_blank_iq_dev
 * would, at the handle's output rate; gyp_ingest_find_tones and gyp_ingest_calibrate then measure the blanked output.  A pulse
 * that a resampler or down-converter of T taps has smeared over T samples is covered by a guard of T / 2.
 * gyp_ingest_set_blanker (NULL: off) follows gyp_ingest_set_level: it takes effect with the next block handed out, and what was
 * uploaded ahead is dropped and read again. */
int gyp_ingest_set_blanker(gyp_ingest* ing, const gyp_blanker* blanker);
int gyp_ingest_get_blanker(const gyp_ingest* ing, gyp_blanker* out, int32_t* enabled_out);
/* Measures output milliseconds [first_ms, first_ms + n_ms) of the handle (inside [0, total_ms), 1 <= n_ms <= 1000) and derives a
 * blanker.  What is measured is the handle's output WITHOUT blanker, notches and level, read through the handle's own path into
 * one buffer, so the result does not depend on block_ms.  The centre is the range's mean -- gyp_iq_stats_dev and the m_re, m_im
 * arithmetic of gyp_iq_level_from_stats, rounded to float32 -- when remove_dc != 0, else 0; then gyp_iq_power_hist_dev about that
 * centre and gyp_blank_from_hist with threshold_over_median and guard.  With install != 0 the blanker is installed as
 * gyp_ingest_set_blanker does.  blanker_out / measured_out2 (either may be NULL) receive what gyp_blank_from_hist wrote.  The
 * cursor is put back, the call synchronises, and blocks handed out earlier are no longer valid afterwards.  On any error the
 * handle keeps what it had: blanker, notches, level and cursor. */
int gyp_ingest_find_pulses(gyp_ingest* ing, int64_t first_ms, int32_t n_ms, int32_t remove_dc, double threshold_over_median, int32_t guard,
                           int32_t install, gyp_blanker* blanker_out, double* measured_out2);
/* The blanked samples per millisecond of the block most recently handed out by gyp_ingest_next_dev: min(cap, its n_ms) counts
 * into counts_out, its n_ms into *n_ms_out (0 before the first block and after a seek).  Zeros while no blanker is on.  The call
 * waits for that block's upload chain only, not for blocks uploaded ahead and not for the context's stream. */
int gyp_ingest_last_blanked(gyp_ingest* ing, int32_t* counts_out, int32_t cap, int32_t* n_ms_out);

/* ---------------------------------------------------------------- excisor: narrowband and swept interference -- */
/* Continuous interference that is narrow but no pure tone -- a carrier with FM or AM on it, a narrowband digital signal, a spur
 * that drifts by kHz per millisecond, a slow swept jammer, more tones than a notch list holds -- passes the notches (a
 * one-millisecond projection onto a fixed frequency cannot follow it) and the blanker (it is always on), and the level then
 * scales the recording by the jammer's power.  The excisor takes short overlapped transforms, zeroes the bins that stand above
 * the noise and subtracts what they held; it adapts every 128 samples and needs no frequency list.  Three steps: a histogram of
 * the bins' power on the device (gyp_iq_spectrum_hist_dev), a threshold from its median on the host (gyp_excise_from_hist), the
 * excision (gyp_excise_iq_dev, or gyp_ingest_set_excisor / gyp_ingest_find_excisor on an ingest handle).  Everything is opt-in:
 * with none of these called every other entry point gives the bits it gave before.
 *
 * Framing.  Per (stream, millisecond of n = samples_per_ms samples), a pure function of that millisecond's samples and the
 * stream's excisor, so blocks, windows, seeks and call shapes give identical samples.  L = GYP_EXCISE_FRAME = 256, hop 128.
 * Frame f covers the millisecond's samples 128 f - 128 .. 128 f + 127; samples outside 0 .. n - 1 are zero; f = 0 .. nf - 1 with
 * nf = ceil((n + 128) / 128): every sample lies in exactly two frames.
 * Analysis.  w[k] = sin^2(pi k / 256) (periodic Hann: w[k] + w[k + 128] = 1), evaluated in float64 and rounded to float32;
 * X_f = FFT256(w x_f), not normalised, in float32;  p_k = re re + im im in float32, one rounding per operation.
 * Decision.  t2 = threshold threshold (one float32 product).  Bin k is a HIT iff p_k >= t2 (equality is a hit; a NaN is not).
 * Bin k is EXCISED iff some hit j has min(|k - j|, 256 - |k - j|) <= guard: the guard is circular, the spectrum wraps at +- fs/2.
 * Removal.  E_f = X_f on the excised bins, 0 elsewhere;  e_f = IFFT256(E_f) / 256.  For sample i with covering frames f < f + 1:
 * c = e_f[i] + e_(f+1)[i] (the lower frame first), y[i] = x[i] - c, float32, no contraction.  A frame without an excised bin
 * contributes nothing (c is then the other frame's term alone), and a sample whose two frames both have none KEEPS ITS BITS, NaN
 * payloads and -0 included; in place such a sample is not written.  The synthesis window is the identity and no re-synthesised
 * copy of the signal is subtracted, only what the excised bins held: no float32 transform error reaches a sample that needed
 * nothing.  The transform's own rounding (a radix-4 float32 transform, about 1e-6 of a frame's norm) is the only freedom an
 * implementation has; decisions within that of t2 may differ between implementations, never between call shapes.
 * Edge cost.  The first and the last frame of a millisecond see half a window of zeros: an interferer is found 3 dB later
 * there, and up to 128 samples at either edge of a millisecond are cleaned less well -- the counterpart of the blanker's guard
 * not crossing millisecond edges.
 * Out of scope.  Fast "privacy device" chirps that cross the whole band within a frame (10 MHz in ~9 us) look broadband in every
 * frame and are not addressed. */
#define GYP_EXCISE_FRAME 256
typedef struct gyp_excisor {      /* one per stream: 16 bytes */
    float threshold;              /* positive, finite: an amplitude of |X_f[k]| */
    int32_t guard;                /* 0..8 bins excised on either side of every hit, round the ring of 256 */
    int32_t reserved[2];          /* must be 0 */
} gyp_excisor;
/* n_ms milliseconds of each of n_streams streams (stream s at sample s * stream_stride_samples of both buffers), stream s with
 * excisors_host[s].  out_dev may equal in_dev (then only corrected samples are written); other overlaps are not allowed.
 * counts_out_dev (may be NULL) receives n_streams x n_ms int32 counts of excised (frame, bin) cells per millisecond, stream-major.
 * masks_out_dev (may be NULL) receives, per (stream, millisecond, frame) in that order, four uint64 words: bit k & 63 of word
 * k >> 6 is set when bin k of the frame was excised -- the interference waterfall.  Any 8-byte aligned address and any stride;
 * rows are read and written 8 bytes per lane, 512 contiguous bytes per wavefront, whatever their alignment.  samples_per_ms is an
 * argument, no stream format is needed.  Enqueued on the context's stream; excisors_host may be reused as soon as the call
 * returns.  GYP_E_BAD_ARG, before anything is launched, for NULL pointers, n_streams < 1, samples_per_ms < 1 or > 65536, n_ms < 0,
 * a stride below n_ms * samples_per_ms when n_streams > 1, a threshold that is not positive and finite, a guard outside 0..8, or
 * reserved words that are not 0. */
int gyp_excise_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                      int32_t samples_per_ms, const gyp_excisor* excisors_host, int32_t* counts_out_dev, uint64_t* masks_out_dev);

/* The histogram of p_k (as above) over n_ms milliseconds of each stream: n_streams x GYP_POWER_HIST_BINS uint32 counts into
 * hist_out_dev, which the call zeroes first.  Binning is that of gyp_iq_power_hist_dev: the bits of p without the sign, shifted
 * right by 20.  Only frames that lie ENTIRELY INSIDE their millisecond are counted (f >= 1 and 128 f + 128 <= n): a frame half
 * of zeros has half the noise power and would pull the median down.  Integer atomics: histograms of parts of a stream add up to
 * the whole's.  Enqueued on the context's stream.  GYP_E_BAD_ARG for NULL pointers, n_streams < 1, n_ms < 1, samples_per_ms < 256
 * or > 65536, or a stride below n_ms * samples_per_ms when n_streams > 1. */
int gyp_iq_spectrum_hist_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                             int32_t samples_per_ms, uint32_t* hist_out_dev);

/* Host only (no GPU; errors through gyp_last_error(NULL)): the excisor whose threshold is sqrt(threshold_over_median x the median
 * of p) from one stream's histogram: the median and t arithmetic of gyp_blank_from_hist, in the same order and with the same
 * roundings.  excisor_out = {(float)t, guard, {0, 0}};  measured_out2 (may be NULL) = {median, t}.  For complex Gaussian noise a
 * bin's power is exponential, so a factor of 16 excises one clean bin in 65536.  GYP_E_BAD_ARG for NULL hist or excisor_out,
 * M = 0, a median that is not positive, a factor that is not positive and finite, a guard outside 0..8, or a threshold that
 * float32 cannot hold. */
int gyp_excise_from_hist(const uint32_t* hist, double threshold_over_median, int32_t guard, gyp_excisor* excisor_out, double* measured_out2);

/* An excisor on an ingest handle (ctx required: a host-only handle returns GYP_E_BAD_ARG from all four, and gyp_ingest_next_host
 * returns GYP_E_BAD_ARG while an excisor is on).  CHAIN ORDER of a handle: producer -> blanker -> excisor -> notches -> level.
 * Every device block is excised in place on the upload stream exactly as gyp_excise_iq_dev would, at the handle's output rate
 * (at most 65536 samples per millisecond).  With an excisor installed, and only then, gyp_ingest_find_tones and
 * gyp_ingest_calibrate measure the EXCISED output.  gyp_ingest_set_excisor (NULL: off) follows gyp_ingest_set_blanker: it takes
 * effect with the next block handed out, and what was uploaded ahead is dropped and read again. */
int gyp_ingest_set_excisor(gyp_ingest* ing, const gyp_excisor* excisor);
int gyp_ingest_get_excisor(const gyp_ingest* ing, gyp_excisor* out, int32_t* enabled_out);
/* Measures output milliseconds [first_ms, first_ms + n_ms) of the handle (inside [0, total_ms), 1 <= n_ms <= 1000; at least 256
 * samples per millisecond) and derives an excisor.  What is measured is the handle's output WITHOUT excisor, notches and level --
 * the blanked output where a blanker is installed -- read through the handle's own path into one buffer, so the result does not
 * depend on block_ms: gyp_iq_spectrum_hist_dev, then gyp_excise_from_hist with threshold_over_median and guard.  With
 * install != 0 the excisor is installed as gyp_ingest_set_excisor does.  excisor_out / measured_out2 (either may be NULL) receive
 * what gyp_excise_from_hist wrote.  The cursor is put back, the call synchronises, and blocks handed out earlier are no longer
 * valid afterwards.  On any error the handle keeps everything it had. */
int gyp_ingest_find_excisor(gyp_ingest* ing, int64_t first_ms, int32_t n_ms, double threshold_over_median, int32_t guard, int32_t install,
                            gyp_excisor* excisor_out, double* measured_out2);
/* The excised (frame, bin) cells per millisecond of the block most recently handed out by gyp_ingest_next_dev: min(cap, its n_ms)
 * counts into counts_out, its n_ms into *n_ms_out (0 before the first block and after a seek).  Zeros while no excisor is on.
 * The call waits for that block's upload chain only. */
int gyp_ingest_last_excised(gyp_ingest* ing, int32_t* counts_out, int32_t cap, int32_t* n_ms_out);

/* ---------------------------------------------------------------- signal quality: C/N0 and carrier lock -- */
/* A receiver reports a carrier-to-noise density per tracked satellite.  gyp_track_rec carries the raw prompt peak and the
 * reference's `locked` flag, whose fixed thresholds depend on the recording's amplitude; C/N0 does not depend on scale, and says
 * what a level or a notch bought.  Two steps: the device reduces a block's records to sums per (channel, window)
 * (gyp_track_quality_dev, on records that are still in HBM behind gyp_track_block_dev), the host turns sums into figures
 * (gyp_quality_from_sums).  Everything is opt-in: with none of these called every other entry point gives the bits it gave before.
 *
 * Windows.  Window w of window_ms = W records covers records [w W, min((w + 1) W, n_ms)) of each channel; n_win = ceil(n_ms / W);
 * the output is n_chan x n_win records, channel-major.  A record is USED iff status != 2 (status 1 is the millisecond that
 * raised: its peak is real).
 *
 * Per record, float64 without contraction:  p2 = (double)re (double)re + (double)im (double)im  (both products exact, the sum one
 * rounding),  p4 = p2 p2.
 *
 * Groups (narrow-band / wide-band power, Van Dierendonck).  For a channel with bit offset b in 0..19, group g >= 0 is the 20
 * records starting at call-relative index b + 20 g.  A group belongs to the window that contains all 20 of its records; one that
 * straddles a window edge or the end of the call belongs to no window.  In record order:  sI = sum (double)re,  sQ = sum
 * (double)im,  WBP = sum p2;  then  NBP = sI sI + sQ sQ,  NBD = sI sI - sQ sQ.  The group is VALID iff all 20 records are used,
 * WBP > 0 and NBP > 0; a valid group contributes NBP / WBP and NBD / NBP (IEEE float64 divisions).  b = -1: no groups (n_groups = 0
 * and both sums 0.0).
 *
 * Order.  One 64-lane wavefront owns a (channel, window).  Lane l adds the used records l, l + 64, ... of the window, in that
 * order, to its accumulators, and owns the window's groups l, l + 64, ... (numbered from the window's first group) in that order;
 * the lanes are reduced by a fixed tree -- lane l takes lane l + 32, 16, 8, 4, 2, 1 -- and lane 0 writes.  No atomics.
 * INVARIANCE: a record is a pure function of its window's records and of the position of the bit edges in it.  The same bits come
 * out for every n_chan split and every chan_stride_recs, and for a call on the sub-range that starts at record w0 W with the bit
 * offsets shifted to (b - w0 W) mod 20.  Non-finite peaks: the sums follow IEEE, the counts are unspecified. */
typedef struct gyp_quality_sums {   /* one per (channel, window): 48 bytes */
    int32_t n_used;      /* records of the window with status != 2 */
    int32_t n_locked;    /* of those, records with locked != 0 */
    int32_t n_groups;    /* valid 20-ms groups */
    int32_t reserved;    /* written 0 */
    double sum_p2;       /* sum of p2 = re*re + im*im over the used records */
    double sum_p4;       /* sum of p2*p2 */
    double sum_np;       /* sum over valid groups of NBP / WBP */
    double sum_pl;       /* sum over valid groups of NBD / NBP */
} gyp_quality_sums;
/* recs_dev: n_chan rows of n_ms records, channel c at record c * chan_stride_recs (gyp_track_block_dev's output: stride n_ms).
 * bit_offset_host: n_chan values in -1..19, or NULL for all -1; they travel as a kernel argument and may be reused as soon as the
 * call returns.  out_dev: n_chan x ceil(n_ms / window_ms) records.  No stream format is needed.  Enqueued on the context's
 * stream.  GYP_E_BAD_ARG for NULL pointers, n_chan < 1, n_ms < 1, window_ms < 1, a stride below n_ms when n_chan > 1, or a bit
 * offset outside -1..19. */
int gyp_track_quality_dev(gyp_ctx* ctx, const gyp_track_rec* recs_dev, int32_t n_chan, int64_t chan_stride_recs, int32_t n_ms,
                          int32_t window_ms, const int32_t* bit_offset_host, gyp_quality_sums* out_dev);
/* The same for records and results in host memory (recs_host spans (n_chan - 1) * chan_stride_recs + n_ms records); synchronous. */
int gyp_track_quality(gyp_ctx* ctx, const gyp_track_rec* recs_host, int32_t n_chan, int64_t chan_stride_recs, int32_t n_ms,
                      int32_t window_ms, const int32_t* bit_offset_host, gyp_quality_sums* out_host);

/* Host only (no GPU; errors through gyp_last_error(NULL)): the figures of n >= 1 records combined -- consecutive windows of one
 * channel, say.  Counts are added as integers, S2, S4, Snp, Spl are the plain left-to-right sums of sum_p2, sum_p4, sum_np, sum_pl.
 * Float64, in exactly this order, one rounding per operation (no contraction).  An estimate that is not defined is NaN: a value,
 * not an error.
 *   Moments (M2M4; needs no bit phase).  NaN if n_used < 2.  n = (double)n_used;  M2 = S2 / n;  M4 = S4 / n;  a = M2 M2;  t = a + a;
 *     d = t - M4;  NaN if !(d > 0);  Pd = sqrt(d);  Pn = M2 - Pd;  NaN if !(Pn > 0);  cn0_m2m4_dbhz = 10 log10((Pd / Pn) 1000.0).
 *     Assumes a constant-modulus signal in complex Gaussian noise.
 *   NWPR.  NaN if n_groups < 1.  G = (double)n_groups;  mu = Snp / G;  NaN if !(mu > 1 && mu < 20);
 *     cn0_nwpr_dbhz = 10 log10(((mu - 1) / (20 - mu)) 1000.0).  Assumes groups that lie inside one data bit: a wrong bit offset
 *     biases it low.
 *   phase_lock = Spl / G: about +1 when the carrier is phase locked, about 0 when it is not; NaN without groups.
 *   locked_share = (double)n_locked / (double)n_used; NaN if n_used = 0.
 * Both C/N0 figures are per 1 ms prompt, hence the factor 1000 (dB-Hz).  GYP_E_BAD_ARG for NULL pointers or n < 1. */
typedef struct gyp_quality {   /* 40 bytes */
    double cn0_m2m4_dbhz, cn0_nwpr_dbhz, phase_lock, locked_share;
    int32_t n_used, n_groups;
} gyp_quality;
int gyp_quality_from_sums(const gyp_quality_sums* sums, int32_t n, gyp_quality* out);

/* A/B switches and test hooks of a context, by name.  The library reads NO environment variable for them (only GYP_RCCL_LIB,
 * a deployment's library path): a stray variable must not change the speed path.  Names, value ranges (checked; GYP_E_BAD_ARG
 * with a message otherwise) and defaults:
 *   "no_pipe" 0/1 (0)           the two-workgroups-per-CU cells kernel instead of the pipelined one; no speculative tracker
 *   "no_shared_fwd" 0/1 (0)     flat grids transform every cell's rows themselves
 *   "no_acq_shared_fwd" 0/1 (0) acquisition levels 1-3 at 8 samples per chip transform every cell's rows themselves (default: one
 *                               forward pass per (stream, Doppler bin) shared by the satellites on that bin; same records); the helper
 *                               contexts of a split scan inherit it
 *   "no_grid_parts" 0/1 (0)     flat-grid work items take whole (unit, satellite group)s even where that leaves the last round of a
 *                               launch partly empty (default: a unit's polyphase branches are cut into runs, merged afterwards)
 *   "no_grid_fused" 0/1 (0)     flat grids that fill the chip (<= 8 samples per chip, single block) fold into rows in HBM first (r05's
 *                               grid_fold_kernel + grid_cells_wave_shared_kernel) instead of one fused kernel per (stream, bin) unit
 *   "grid_fused_waves" 8 or 12 (12)  wavefronts per workgroup of the fused flat-grid kernel: 12 = three per SIMD at <= 170 registers (the replica
 *                               multiplied in from L1 / L2 in batches), 8 = two per SIMD at 256 (the next replica prefetched into registers); same cells
 *   "last_grid_path" (read only, gyp_debug_get)  the cells kernel the last gyp_correlate_grid* call took: 1 fused, 2 shared forward
 *                               transforms out of folded rows, 3 one wavefront per cell, 4 one workgroup per cell
 *   "last_acq_units", "last_acq_shared_cells", "last_acq_unshared_cells" (read only, gyp_debug_get)  what the levels of the last
 *                               gyp_acquire(_dev) / gyp_search_level(_dev) on the context did, summed over its levels: (stream, Doppler bin) units
 *                               given one forward pass of their own, cells that read a unit's spectra, cells on the unshared work list (every
 *                               correlated cell is one or the other); "<name>_l<k>", k = 1..16: level k alone.  Counted on the device by the
 *                               work-list kernels; the scan itself copies and waits for nothing -- gyp_debug_get waits for the context's stream
 *                               (and its helpers') and copies then.  The caller's context reports its own part plus the parts its helper
 *                               contexts ran.  With "no_acq_shared_fwd" 1, at rates other than 8 samples per chip and from level 4 on the first two are 0
 *   "spec_sub_ms" 0, 100..2000 (0)  target length of the sub-blocks of a speculative tracking block (a failed verification costs its
 *                               channel one); 0: by rate -- 167 ms at 2.046 Msps, 500 ms otherwise
 *   "no_acq_split" 0/1 (0)      a multi-stream scan runs on the caller's stream alone
 *   "acq_lanes" 1..4 (2)        parts a multi-stream scan is split into
 *   "cells_cu_reserve" 0..128 (0)  CUs the correlation-cell launches of this context leave free (a receiver's scan context beside its
 *                               one-CU-per-channel trackers: 16 = two per XCD); same results, the cells are walked grid-stride
 *   "no_spec" 0/1 (0)           lightly loaded banks use the throughput kernel too
 *   "spec_redo" 0/1 (1)         0: a failed speculation is re-run on the throughput kernel (r03 behaviour)
 *   "spec_debug" 0/1 (0)        per-ms window dump for gyp_debug_spec_read
 *   "track_chunk_ms" 0 | >= 20 (250)   launch length of the throughput tracking kernel (0: whole blocks)
 *   "resample_tile_samples" 1024..8192 (4096)  LDS budget of one resampler workgroup, in input samples; same output for any value
 *   "notch_no_lds" 0/1 (0)      gyp_notch_iq_dev and the ingest's notches keep the millisecond's residual in the output buffer (the
 *                               form rates above 16.384 Msps take) instead of LDS; same samples bit for bit
 *   "widen_wg_per_cu" 1..8 (2)  workgroups per CU of the widen kernel's persistent grid (gyp_widen_iq_dev, the ingest ring; the unpack,
 *                               statistics and condition kernels follow it); same output for any value
 *   "no_exact_shared" 0/1 (0)   the exact code-loop sums behind the throughput tracking kernel fetch and convert a stream's samples once per
 *                               channel again (dll_exact_wave_kernel).  Default at 8 samples per chip, plain gyp_track_block(_dev) calls on the
 *                               throughput path: the channels are grouped by stream on the device and each (stream, millisecond) is staged once, as
 *                               float64 in LDS, for up to twelve channels (dll_exact_shared_kernel); same sums bit for bit.  Other rates, the
 *                               speculative tracker's rounds and its re-runs keep the per-channel kernels either way
 *   "last_exact_path" (read only, gyp_debug_get)  the exact-sums kernel of the context's last plain throughput call: 0 none yet,
 *                               1 dll_exact_wave_kernel, 2 dll_exact_shared_kernel, 3 dll_exact_block_kernel (more than 8 samples per chip)
 *   "last_track_flow" (read only, gyp_debug_get)  what the context's last gyp_track_block(_dev) call ran: 0 none yet, 1 the throughput
 *                               kernel, 2 the speculative tracker with the failed channels re-run at the end of the block, 3 the speculative
 *                               tracker under the round protocol
 *   "last_acq_lanes", "last_acq_levels", "last_acq_shared_levels" (read only, gyp_debug_get)  what the context's last gyp_acquire(_dev) /
 *                               gyp_search_level(_dev) call ran (0 none yet): the parts it actually went through in (this context and that many
 *                               helper contexts less one; 1 for a single level), its levels (10 with the default parameters, 1 for a single
 *                               level), and how many of the first of them went through the shared-forward kernels (3 of a scan at 8 samples
 *                               per chip; 0 at other rates, with "no_pipe" or "no_acq_shared_fwd" 1 and beyond 8192 ms)
 *   "track_finish_all" 0/1 (0)  the throughput tracking kernel at up to 8 samples per chip: every wavefront of a channel's workgroup merges the
 *                               millisecond's profile candidates for itself again.  Default: only the wavefronts that use the merged
 *                               profile do (the Costas loop's and the record's), in straight-line code, and the code loop's reads its two
 *                               taps; same records, states and dumps bit for bit.  Rates above 8 samples per chip ignore it; the helper
 *                               contexts of a split scan inherit it
 *   "hybrid_scratch_mb" 16..65536 (1024)  budget, in MiB, of the profile + power scratch of gyp_correlate_grid_hybrid(_dev) and
 *                               gyp_acquire_weak(_dev): the cells go through in chunks that fit it; same records bit for bit
 *   "last_hybrid_chunks" (read only, gyp_debug_get)  chunks of the context's last hybrid grid (of gyp_acquire_weak: its last level's); 0 none yet
 *   "prof_wave" 0..7 (0)        which wavefront of workgroup 0 stamps the counters of gyp_debug_track_profile
 *   "symbol_tau" 0..100 (1e-4)  |Re peak| / |peak| below which dll_scan_kernel decides the pseudosymbol in float64 (test: 10 = always)
 *   "dll_prov_bias" (0)         test hook: added to the PROVISIONAL discriminator so that the repair path runs; results must not change
 *   "spec_fail_at" >= -1 (-1)   test hook: channel 0's verification is made to fail at that millisecond of a block
 * Helper contexts of a split scan inherit the caller's values. */
int gyp_debug_set(gyp_ctx* ctx, const char* name, double value);
int gyp_debug_get(gyp_ctx* ctx, const char* name, double* value_out);
/* Debug: per-phase shader-cycle counters of workgroup 0 of gyp_track_block_dev (correlate, reduce, loop update,
 * barrier, ms count) or, for the pipelined 8.184 Msps non-coherent cells kernel behind gyp_correlate_cells_dev /
 * gyp_acquire_dev, (stage, row load + forward, spectrum + prefetch, inverse + accumulate, barrier, iterations).
 * enable != 0 arms it; out16 (may be NULL, else room for 16 values) receives the counters of the last launch: [0..4] as
 * above, [5] milliseconds that took the transform path in the speculative tracker, [6..15] the speculative tracker's
 * stamp-to-stamp cycles (state read, sample requests, staging, boundary sums, barrier, window, barrier, decision,
 * transform path if taken, loop update). */
int gyp_debug_track_profile(gyp_ctx* ctx, int enable, long long* out16);
/* Debug (speculative block tracker: 8.184 / 2.046 Msps banks of at most one channel per CU): after
 * gyp_debug_set(ctx, "spec_debug", 1) the last gyp_track_block(_dev) call leaves, per (channel, ms), 20 floats: |c0|^2 at the 8 window lags
 * (previous peak lag - 4 .. + 3), 8 zeros, the sample-energy estimate, code_phase mod N, the window centre, 0.  bad_out (may be NULL): per
 * channel, 1 if the verify pass sent the channel back through the transform kernel.  Synchronises the stream. */
int gyp_debug_spec_read(gyp_bank* bank, float* out, int32_t n_floats, int32_t* bad_out);
/* Debug / measurement: HIP events on the context's stream around the three stages behind gyp_track_block(_dev) on the
 * throughput path (banks of more than one channel per CU): enable != 0 arms it; out4 (may be NULL) receives, for the last
 * call, {ms in track_block_kernel (all its launches), ms in the dll_exact kernel (with dll_exact_shared_kernel: its grouping kernel too), ms in dll_scan_kernel, number of
 * track_block_kernel launches: blocks longer than 250 ms go through in chunks, gyp_debug_set "track_chunk_ms"} -- zeros when that call
 * ran on the speculative path (lightly loaded banks), which has no such split.  bench.py's per-kernel roofline uses it. */
int gyp_debug_track_timing(gyp_ctx* ctx, int enable, float* out4);
/* Debug / telemetry (either tracking path): repairs_out[n_chan] = milliseconds of the last gyp_track_block(_dev) call in which
 * the exactly re-integrated code loop (dll_scan_kernel) had int(self.phase) differ from the tracking kernel's provisional one
 * and formed that millisecond's float64 sums again for the right lag.  Synchronises the stream. */
int gyp_debug_dll_read(gyp_bank* bank, int32_t* repairs_out);
/* Debug (throughput path): disc_out[n_chan][n_ms] = the float64 discriminators (tracker.py:297) the exact-sums kernel formed for the
 * bank's last gyp_track_block(_dev) call, at the lag the tracking kernel ran each millisecond with -- dll_scan_kernel's input, before
 * any repair; milliseconds a lost channel did not process read 0.  n_ms must be that call's length (GYP_E_BAD_ARG otherwise, or if the
 * bank has not tracked a block on the throughput path).  Synchronises the stream. */
int gyp_debug_disc_read(gyp_bank* bank, int32_t n_ms, double* disc_out);
/* Debug / telemetry (speculative block tracker): out4 = {sub-blocks of the last gyp_track_block(_dev) call, rounds enqueued for it,
 * sub-blocks tracked AGAIN from their checkpoint because a millisecond's window had not held the profile's arg-max (the failed
 * millisecond then takes the transform path), channels finished by the transform kernel instead (out of forced-transform slots or
 * of rounds; every failure went this way up to ABI 200)}.  Zeros if the bank never took the speculative path.  Synchronises the stream. */
int gyp_debug_spec_redo_read(gyp_bank* bank, int32_t* out4);
/* Debug (host arithmetic only, no device needed): the sub-blocks the speculative tracker cuts a block of n_ms milliseconds into --
 * starts_out[0 .. n] with starts_out[n] = n_ms, n <= 32 returned (sub-block s is [starts_out[s], starts_out[s + 1])); long blocks end
 * with shrinking sub-blocks because only the LAST sub-block's verification is not hidden behind tracking.
 * starts_out must hold 33 values.  Returns n, or GYP_E_BAD_ARG (negative). */
int gyp_debug_spec_layout(int32_t n_ms, int32_t* starts_out);
/* The same for a target sub-block length of sub_ms (100..2000): what a context at 2.046 Msps uses (167) against 500 elsewhere -- at two
 * samples per chip a millisecond is cheap and a failed verification should cost few of them ("spec_sub_ms" of gyp_debug_set overrides). */
int gyp_debug_spec_layout_for(int32_t n_ms, int32_t sub_ms, int32_t* starts_out);
/* Debug: time `iters` forward+inverse wavefront transform pairs per wavefront, `wgs` workgroups of `waves_per_wg`
 * wavefronts (LDS-resident data, no global traffic): the floor the correlator kernels are measured against. */
int gyp_debug_fft_bench(gyp_ctx* ctx, int waves_per_wg, int wgs, int iters, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* GYPSUM_HIP_H */
